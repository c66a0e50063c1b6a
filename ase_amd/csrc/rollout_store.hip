// One environment step of the rollout loop stored by ONE entry: the block of CommonAgent.play_steps behind
// env_step (learning/common_agent.py:267-293 of the reference; amp_agent.py:93-122, ase_agent.py:66-100, hrl_agent.py:124-151) -
// the copies into experience slot n, the shaped reward, the masked next value, the episode accumulators, the two AverageMeter
// updates and the list of done rows - without dones.nonzero(): the contract is ase_hip_rollout_store's in include/ase_hip.h.
// Two launches: the store kernel leaves one partial {sum of returns, sum of lengths, done rows} per block in the caller's
// workspace with plain stores, a one-wave kernel folds them in a fixed order into the meter (no floating-point atomics, no
// ticket: a kernel boundary orders the two, as in ase_hip_ppo_head).
#include "common.h"

namespace {

constexpr int kRows = ASE_ROLLOUT_STORE_ROWS;    // environments per block, two per wave: 512 blocks at 4096 environments
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct RolloutStoreArgs {
    const int64_t* fields;                       // DEVICE [n_fields][6] = {src, ld_src, D, dst_base, ld_dst, slot_stride}
    const float* rewards;
    float* rewards_out;
    const void* dones;
    uint8_t* dones_out;
    const float* next_values;
    const void* terminate;
    float* next_values_out;
    float* cur_rewards;
    float* cur_lengths;
    double* meter;
    double* ws;                                  // [blocks][3]
    int32_t* done_ids_out;
    const int32_t* slot_dev;
    int64_t rewards_ss, dones_ss, next_values_ss;
    float shift, scale;
    int n_fields, dones_kind, terminate_kind, max_size, n_envs, slot, n_slots;
};

// the slot a launch writes: the device word when there is one (read when the launch runs), -1 when it names no slot
__device__ __forceinline__ int store_slot(const int32_t* slot_dev, int slot, int n_slots) {
    if (!slot_dev) return slot;
    const int s = *slot_dev;
    return s >= 0 && s < n_slots ? s : -1;
}

// Block b owns rows [b kRows, (b + 1) kRows).  Lanes 0 .. kRows - 1 do a row's scalar work each; then every field's rows are
// copied a wave per row, consecutive lanes on consecutive columns (16 bytes per lane where the field allows it).
__global__ __launch_bounds__(kThreads) void rollout_store_kernel(RolloutStoreArgs a) {
    __shared__ double part_r[kRows], part_l[kRows];
    __shared__ int part_k[kRows];
    const int slot = store_slot(a.slot_dev, a.slot, a.n_slots);
    if (slot < 0) return;                                    // a slot word outside the buffer: nothing is written
    const int tid = threadIdx.x, r0 = blockIdx.x * kRows;
    const int nrows = min(kRows, a.n_envs - r0);
    if (tid < kRows) {
        double pr = 0.0, pl = 0.0;
        int pk = 0;
        if (tid < nrows) {
            const int e = r0 + tid;
            bool done;
            const float d = flag_value(a.dones, a.dones_kind, e, done);
            if (a.dones_out) a.dones_out[slot * a.dones_ss + e] = done ? 1 : 0;
            if (a.done_ids_out) a.done_ids_out[e] = done ? e : -1;
            if (a.rewards_out) a.rewards_out[slot * a.rewards_ss + e] = (a.rewards[e] + a.shift) * a.scale;
            if (a.next_values_out) {
                bool t_set;
                const float t = flag_value(a.terminate, a.terminate_kind, e, t_set);
                a.next_values_out[slot * a.next_values_ss + e] = a.next_values[e] * (1.0f - t);
            }
            if (a.cur_rewards) {
                const float r = a.cur_rewards[e] + a.rewards[e];             // the raw reward, not the shaped one
                const float l = a.cur_lengths[e] + 1.0f;
                if (done) { pr = (double)r; pl = (double)l; pk = 1; }
                const float keep = 1.0f - d;
                a.cur_rewards[e] = r * keep;
                a.cur_lengths[e] = l * keep;
            }
        }
        part_r[tid] = pr; part_l[tid] = pl; part_k[tid] = pk;
    }
    __syncthreads();
    if (tid == 0 && a.ws) {                                  // the block's partial, its rows in order
        double sr = 0.0, sl = 0.0;
        int k = 0;
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            if (part_k[i]) { sr += part_r[i]; sl += part_l[i]; ++k; }
        }
        double* w = a.ws + 3 * (int64_t)blockIdx.x;
        w[0] = sr; w[1] = sl; w[2] = (double)k;
    }
    const int lane = tid & 63, wave = tid >> 6;
    for (int f = 0; f < a.n_fields; ++f) {
        const int64_t* d = a.fields + 6 * f;
        const float* src = reinterpret_cast<const float*>(d[0]);
        const int64_t ld_src = d[1], ld_dst = d[4], ss = d[5];
        const int D = (int)d[2];
        float* dst = reinterpret_cast<float*>(d[3]) + slot * ss;
        // 16 bytes per lane: whole chunks in every row of both sides (ase_hip_rollout_store's condition in the header)
        const bool vec = D % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && ss % 4 == 0 && ((uintptr_t)src & 15) == 0 &&
                         ((uintptr_t)d[3] & 15) == 0;
        for (int rr = wave; rr < nrows; rr += kWaves) {
            const float* s = src + (int64_t)(r0 + rr) * ld_src;
            float* o = dst + (int64_t)(r0 + rr) * ld_dst;
            if (vec) {
#pragma unroll 2
                for (int c = lane; c < D / 4; c += 64)
                    reinterpret_cast<uint4*>(o)[c] = reinterpret_cast<const uint4*>(s)[c];
            } else {
#pragma unroll 2
                for (int c = lane; c < D; c += 64)
                    reinterpret_cast<uint32_t*>(o)[c] = reinterpret_cast<const uint32_t*>(s)[c];
            }
        }
    }
}

// One wave: lane i adds the partials of blocks i, i + 64, ... in that order, a butterfly adds the 64 lane sums - the same
// order on every run.  Then AverageMeter.update (rl_games torch_ext) for both meters, in f64.
__global__ __launch_bounds__(64) void rollout_meter_kernel(const double* __restrict__ ws, int blocks, double* __restrict__ meter,
                                                           int max_size, const int32_t* slot_dev, int n_slots) {
    if (store_slot(slot_dev, 0, n_slots) < 0) return;
    double v[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < blocks; b += 64) {
        const double k = ws[3 * (int64_t)b + 2];
        if (k != 0.0) { v[0] += ws[3 * (int64_t)b]; v[1] += ws[3 * (int64_t)b + 1]; v[2] += k; }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = wave_sum(v[i]);
    if (threadIdx.x != 0 || v[2] == 0.0) return;             // no done row: the meter is not touched
    const double k = v[2];
    const double size = k < (double)max_size ? k : (double)max_size;
    const double room = (double)max_size - size, cur = meter[2];
    const double old = room < cur ? room : cur;
    const double size_sum = old + size;
    meter[0] = (meter[0] * old + (v[0] / k) * size) / size_sum;
    meter[1] = (meter[1] * old + (v[1] / k) * size) / size_sum;
    meter[2] = size_sum;
    meter[3] += k;
}

}  // namespace

extern "C" int ase_hip_rollout_store(const int64_t* fields, int n_fields, const float* rewards, float shift, float scale,
                                     float* rewards_out, int64_t rewards_ss, const void* dones, int dones_kind,
                                     uint8_t* dones_out, int64_t dones_ss, const float* next_values, const void* terminate,
                                     int terminate_kind, float* next_values_out, int64_t next_values_ss, float* cur_rewards,
                                     float* cur_lengths, double* meter, int max_size, double* workspace,
                                     int64_t workspace_doubles, int32_t* done_ids_out, int n_envs, int slot,
                                     const int32_t* slot_dev, int n_slots, void* stream) {
    ASE_CHECK_ARG(dones, "rollout_store: null dones");
    ASE_CHECK_ARG(n_envs > 0, "rollout_store: n_envs %d", n_envs);
    ASE_CHECK_ARG(n_fields >= 0 && n_fields <= ASE_ROLLOUT_STORE_MAX_FIELDS, "rollout_store: n_fields %d outside [0, %d]", n_fields,
                  ASE_ROLLOUT_STORE_MAX_FIELDS);
    ASE_CHECK_ARG(fields || n_fields == 0, "rollout_store: %d fields without a table", n_fields);
    ASE_CHECK_ARG(kind_ok(dones_kind), "rollout_store: dones kind %d (ASE_KIND_U8 / I32 / I64 / F32)", dones_kind);
    const bool acc_any = cur_rewards || cur_lengths || meter || workspace;
    const bool acc_all = cur_rewards && cur_lengths && meter && workspace;
    ASE_CHECK_ARG(acc_any == acc_all, "rollout_store: partial accumulator group (cur_rewards, cur_lengths, meter, workspace come "
                  "together)");
    ASE_CHECK_ARG(!rewards_out || rewards, "rollout_store: partial rewards group (rewards_out without rewards)");
    ASE_CHECK_ARG(!acc_all || rewards, "rollout_store: the accumulators need rewards");
    ASE_CHECK_ARG(!rewards || rewards_out || acc_all, "rollout_store: partial rewards group (rewards without rewards_out or "
                  "accumulators)");
    const bool nv_any = next_values || terminate || next_values_out, nv_all = next_values && terminate && next_values_out;
    ASE_CHECK_ARG(nv_any == nv_all, "rollout_store: partial next_values group (next_values, terminate, next_values_out come "
                  "together)");
    ASE_CHECK_ARG(!nv_all || kind_ok(terminate_kind), "rollout_store: terminate kind %d (ASE_KIND_U8 / I32 / I64 / F32)",
                  terminate_kind);
    ASE_CHECK_ARG((!rewards_out || rewards_ss >= n_envs) && (!dones_out || dones_ss >= n_envs) &&
                      (!nv_all || next_values_ss >= n_envs), "rollout_store: a slot stride below n_envs %d", n_envs);
    ASE_CHECK_ARG(!acc_all || max_size > 0, "rollout_store: max_size %d with a meter", max_size);
    ASE_CHECK_ARG(!acc_all || workspace_doubles >= ASE_ROLLOUT_STORE_WS(n_envs), "rollout_store: workspace of %lld doubles, %d "
                  "needed", (long long)workspace_doubles, ASE_ROLLOUT_STORE_WS(n_envs));
    ASE_CHECK_ARG(n_slots > 0 && slot >= 0 && slot < n_slots, "rollout_store: slot %d outside [0, %d)", slot, n_slots);
    RolloutStoreArgs a = {};
    a.fields = fields; a.n_fields = n_fields;
    a.rewards = rewards; a.rewards_out = rewards_out; a.rewards_ss = rewards_ss; a.shift = shift; a.scale = scale;
    a.dones = dones; a.dones_kind = dones_kind; a.dones_out = dones_out; a.dones_ss = dones_ss;
    a.next_values = next_values; a.terminate = terminate; a.terminate_kind = terminate_kind;
    a.next_values_out = next_values_out; a.next_values_ss = next_values_ss;
    a.cur_rewards = cur_rewards; a.cur_lengths = cur_lengths; a.meter = meter; a.ws = workspace; a.max_size = max_size;
    a.done_ids_out = done_ids_out; a.n_envs = n_envs; a.slot = slot; a.slot_dev = slot_dev; a.n_slots = n_slots;
    const int blocks = (n_envs + kRows - 1) / kRows;
    ASE_LAUNCH(rollout_store_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    if (acc_all) ASE_LAUNCH(rollout_meter_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, workspace, blocks, meter, max_size,
                            slot_dev, n_slots);
    ASE_CHECK_LAUNCH("rollout_store");
    return ASE_OK;
}
