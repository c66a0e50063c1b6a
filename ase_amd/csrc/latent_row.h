// One latent row on one wave (rollout.hip, latent_renew.hip): lanes j and j + 64 hold elements j and j + 64 of a row of
// dim <= 128; the row's normals -> its norm -> the divide, i.e. torch.nn.functional.normalize(N(0, I), dim=-1)
// (learning/ase_network_builder.py:221-225), and the store of a converted second copy.
#pragma once
#include "philox.h"

namespace {

// max(x, lo) as torch.maximum / clamp_min have it: a NaN x stays NaN (fmaxf would return lo)
__device__ __forceinline__ float floor_keep_nan(float x, float lo) { return x < lo ? lo : x; }

// v[q] = normal of stream element first + lane + 64 q (0 where the column is past dim)
__device__ __forceinline__ void latent_row_normals(uint64_t seed, uint64_t off, uint64_t first, int dim, int lane, float (&v)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = lane + 64 * q;
        v[q] = j < dim ? philox_normal(seed, off, first + j) : 0.f;
    }
}

// v / max(|v|, 1e-12) over the wave's row; every lane of the wave calls it
__device__ __forceinline__ void latent_row_normalize(float (&v)[2]) {
    const float nrm = floor_keep_nan(sqrtf(wave_sum(v[0] * v[0] + v[1] * v[1])), 1e-12f);
    v[0] = v[0] / nrm;
    v[1] = v[1] / nrm;
}

// element i of the second copy in its storage type
__device__ __forceinline__ void latent_store_as(void* z2, int z2_dtype, int64_t i, float o) {
    if (z2_dtype == ASE_BF16) reinterpret_cast<bf16_t*>(z2)[i] = (bf16_t)o;
    else if (z2_dtype == ASE_F16) reinterpret_cast<f16_t*>(z2)[i] = from_f32<f16_t>(o);
    else reinterpret_cast<float*>(z2)[i] = o;
}

}  // namespace
