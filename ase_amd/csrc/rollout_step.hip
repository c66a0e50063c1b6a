// The head of one environment step of the rollout loop as ONE launch, and the step counter of a
// recorded rollout step.  ase_hip_rollout_head replaces, on a raw observation, the obses copy into the experience slot
// (learning/common_agent.py:253-262 of the reference), the eval-mode normalisation into the actor's and the critic's input
// buffers (rms_normalize_kernel, rms.hip:197-203) and the two latent gathers (gather_rows_kernel, rms.hip:257); the contract is
// ase_hip_rollout_head's in include/ase_hip.h.  ase_hip_word_step advances the device word the head and ase_hip_rollout_store
// read their slot from.  Compiled without a * b + c contraction, like rms.hip.
#include "common.h"

namespace {

constexpr int kRows = 8;                         // rows per block, two per wave: 512 blocks at 4096 environments
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct RolloutHeadArgs {
    const float* obs;  int64_t ld_obs;
    const float* z;    int64_t ld_z;
    const float* mean; const float* stdv;
    void* xa;          int64_t ld_xa;
    void* xc;          int64_t ld_xc;
    void* zc;          int64_t ld_zc;
    void* zs;          int64_t ld_zs;
    float* obses_out;  int64_t ld_oo, ss_oo;
    float* z_out;      int64_t ld_zo, ss_zo;
    const int32_t* slot_dev;
    int n, D, Z, slot, n_slots, vec_obs, vec_z;
};

// the one line of rms_normalize_kernel (rms.hip:198-199): an IEEE subtraction, an IEEE division, torch.clamp with a NaN kept
__device__ __forceinline__ float normalized(float x, float mu, float sd) {
    const float y = (x - mu) / sd;
    return ceil_nan(floor_nan(y, -5.f), 5.f);
}

template <typename T, bool PLAIN> __device__ __forceinline__ void store4(void* base, int64_t off, f32x4 y) {
    if (!base) return;
    if constexpr (sizeof(T) == 2) {
        typename V16<T>::x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = PLAIN ? from_f32_plain<T>(y[c]) : from_f32<T>(y[c]);
        *reinterpret_cast<typename V16<T>::x4*>(reinterpret_cast<T*>(base) + off) = v;
    } else {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(base) + off) = y;
    }
}
template <typename T, bool PLAIN> __device__ __forceinline__ void store1(void* base, int64_t off, float y) {
    if (base) reinterpret_cast<T*>(base)[off] = PLAIN ? from_f32_plain<T>(y) : from_f32<T>(y);
}

// Block b owns rows [b kRows, (b + 1) kRows), a wave per row, consecutive lanes on consecutive columns: the observation's
// columns first (raw copy, normalised into xa / xc), then the latent's (raw copy, converted into zc / zs).
template <typename T>
__global__ __launch_bounds__(kThreads) void rollout_head_kernel(RolloutHeadArgs a) {
    int slot = a.slot;
    if (a.slot_dev) {                                        // the word read when the launch runs
        slot = *a.slot_dev;
        if (slot < 0 || slot >= a.n_slots) return;           // a slot word outside the buffer: nothing is written
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * kRows, nrows = min(kRows, a.n - r0);
    const bool norm = a.xa || a.xc;
    float* oo = a.obses_out ? a.obses_out + slot * a.ss_oo : nullptr;
    float* zo = a.z_out ? a.z_out + slot * a.ss_zo : nullptr;
    for (int rr = wave; rr < nrows; rr += kWaves) {
        const int64_t e = r0 + rr;
        const float* src = a.obs + e * a.ld_obs;
        if (a.vec_obs) {
            for (int j = lane * 4; j < a.D; j += 256) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(src + j);
                if (oo) *reinterpret_cast<f32x4*>(oo + e * a.ld_oo + j) = x;
                if (norm) {
                    const f32x4 mu = *reinterpret_cast<const f32x4*>(a.mean + j), sd = *reinterpret_cast<const f32x4*>(a.stdv + j);
                    f32x4 y;
#pragma unroll
                    for (int c = 0; c < 4; ++c) y[c] = normalized(x[c], mu[c], sd[c]);
                    store4<T, true>(a.xa, e * a.ld_xa + j, y);
                    store4<T, true>(a.xc, e * a.ld_xc + j, y);
                }
            }
        } else {
            for (int j = lane; j < a.D; j += 64) {
                const uint32_t bits = reinterpret_cast<const uint32_t*>(src)[j];
                if (oo) reinterpret_cast<uint32_t*>(oo + e * a.ld_oo)[j] = bits;
                if (norm) {
                    const float y = normalized(__builtin_bit_cast(float, bits), a.mean[j], a.stdv[j]);
                    store1<T, true>(a.xa, e * a.ld_xa + j, y);
                    store1<T, true>(a.xc, e * a.ld_xc + j, y);
                }
            }
        }
        if (a.Z <= 0) continue;
        const float* zr = a.z + e * a.ld_z;
        if (a.vec_z) {
            for (int k = lane * 4; k < a.Z; k += 256) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(zr + k);
                if (zo) *reinterpret_cast<f32x4*>(zo + e * a.ld_zo + k) = v;
                store4<T, false>(a.zc, e * a.ld_zc + k, v);
                store4<T, false>(a.zs, e * a.ld_zs + k, v);
            }
        } else {
            for (int k = lane; k < a.Z; k += 64) {
                const uint32_t bits = reinterpret_cast<const uint32_t*>(zr)[k];
                if (zo) reinterpret_cast<uint32_t*>(zo + e * a.ld_zo)[k] = bits;
                const float v = __builtin_bit_cast(float, bits);
                store1<T, false>(a.zc, e * a.ld_zc + k, v);
                store1<T, false>(a.zs, e * a.ld_zs + k, v);
            }
        }
    }
}

// one lane; the sum in 64 bits so that the modulo sees the mathematical value, a plain vector store
__global__ __launch_bounds__(64) void word_step_kernel(int32_t* word, int add, int wrap) {
    if (threadIdx.x != 0) return;
    int64_t v = (int64_t)*word + (int64_t)add;
    if (wrap > 0) {
        v %= (int64_t)wrap;
        if (v < 0) v += wrap;
    }
    *word = (int32_t)(uint32_t)(uint64_t)v;
}

inline bool aligned(const void* p, int bytes) { return ((uintptr_t)p % (uintptr_t)bytes) == 0; }

}  // namespace

extern "C" int ase_hip_rollout_head(const float* obs, int64_t ld_obs, int D, const float* z, int64_t ld_z, int Z, const float* mean,
                                    const float* stdv, void* xa, int64_t ld_xa, void* xc, int64_t ld_xc, void* zc, int64_t ld_zc,
                                    void* zs, int64_t ld_zs, int x_dtype, float* obses_out, int64_t ld_obses_out,
                                    int64_t obses_slot_stride, float* z_out, int64_t ld_z_out, int64_t z_slot_stride, int n, int slot,
                                    const int32_t* slot_dev, int n_slots, void* stream) {
    ASE_CHECK_ARG(xa || xc || zc || zs || obses_out || z_out, "rollout_head: no output at all");
    ASE_CHECK_ARG(n > 0 && D > 0, "rollout_head: n %d, D %d", n, D);
    ASE_CHECK_ARG(obs, "rollout_head: null obs");
    ASE_CHECK_ARG(Z >= 0 && (Z == 0 || z), "rollout_head: Z %d without z", Z);
    ASE_CHECK_ARG(Z > 0 || !(z_out || zc || zs), "rollout_head: a latent output (z_out, zc, zs) with Z == 0");
    ASE_CHECK_ARG(!(xa || xc) || (mean && stdv), "rollout_head: xa / xc without mean and std");
    ASE_CHECK_ARG(x_dtype == ASE_F32 || x_dtype == ASE_BF16 || x_dtype == ASE_F16, "rollout_head: bad x_dtype %d", x_dtype);
    ASE_CHECK_ARG(ld_obs >= D && (!xa || ld_xa >= D) && (!xc || ld_xc >= D) && (!obses_out || ld_obses_out >= D),
                  "rollout_head: a pitch below D %d", D);
    ASE_CHECK_ARG(Z == 0 || (ld_z >= Z && (!zc || ld_zc >= Z) && (!zs || ld_zs >= Z) && (!z_out || ld_z_out >= Z)),
                  "rollout_head: a pitch below Z %d", Z);
    const bool slotted = obses_out || z_out;
    if (slotted) {
        ASE_CHECK_ARG(n_slots > 0 && slot >= 0 && slot < n_slots, "rollout_head: slot %d outside [0, %d)", slot, n_slots);
        ASE_CHECK_ARG((!obses_out || obses_slot_stride >= (int64_t)n * ld_obses_out) && (!z_out || z_slot_stride >= (int64_t)n * ld_z_out),
                      "rollout_head: a slot stride below n * pitch (n %d)", n);
    }
    const int es = ase_elem_size(x_dtype);
    auto x_ok = [&](const void* p, int64_t ld) { return !p || (ld % 4 == 0 && aligned(p, 4 * es)); };
    auto f_ok = [&](const void* p, int64_t ld, int64_t ss) { return !p || (ld % 4 == 0 && ss % 4 == 0 && aligned(p, 16)); };
    RolloutHeadArgs a = {};
    a.obs = obs; a.ld_obs = ld_obs; a.z = Z > 0 ? z : nullptr; a.ld_z = ld_z; a.mean = mean; a.stdv = stdv;
    a.xa = xa; a.ld_xa = ld_xa; a.xc = xc; a.ld_xc = ld_xc; a.zc = zc; a.ld_zc = ld_zc; a.zs = zs; a.ld_zs = ld_zs;
    a.obses_out = obses_out; a.ld_oo = ld_obses_out; a.ss_oo = obses_slot_stride;
    a.z_out = z_out; a.ld_zo = ld_z_out; a.ss_zo = z_slot_stride;
    a.slot_dev = slotted ? slot_dev : nullptr;               // with neither slot output the slot arguments are ignored
    a.n = n; a.D = D; a.Z = Z; a.slot = slotted ? slot : 0; a.n_slots = n_slots;
    // 16 bytes per lane: whole chunks in every row of every operand of that side (the condition in the header)
    a.vec_obs = D % 4 == 0 && ld_obs % 4 == 0 && aligned(obs, 16) && (!(xa || xc) || (aligned(mean, 16) && aligned(stdv, 16))) &&
                x_ok(xa, ld_xa) && x_ok(xc, ld_xc) && f_ok(obses_out, ld_obses_out, obses_slot_stride);
    a.vec_z = Z > 0 && Z % 4 == 0 && ld_z % 4 == 0 && aligned(z, 16) && x_ok(zc, ld_zc) && x_ok(zs, ld_zs) &&
              f_ok(z_out, ld_z_out, z_slot_stride);
    const int blocks = (n + kRows - 1) / kRows;
    ase_dispatch_storage(x_dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        ASE_LAUNCH(rollout_head_kernel<T>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
        return ASE_OK;
    });
    ASE_CHECK_LAUNCH("rollout_head");
    return ASE_OK;
}

extern "C" int ase_hip_word_step(int32_t* word, int add, int wrap, void* stream) {
    ASE_CHECK_ARG(word, "word_step: null word");
    ASE_LAUNCH(word_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, word, add, wrap);
    ASE_CHECK_LAUNCH("word_step");
    return ASE_OK;
}
