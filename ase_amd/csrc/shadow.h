// Compute-dtype shadows of an f32 master weight W [n_real, k_real]: W_s (row-major) and W_s^T (through an LDS transpose), the
// destination column of a concat input shifted past its gap.  One 32 x 32 tile routine for the refresh kernels and the fused
// optimizer launch (optim.hip).  Device code only.
#pragma once
#include "common.h"

// destination column of source column k: a concat input's second part starts `gap` columns further on
__device__ __forceinline__ int shadow_col(int k, int split_src, int gap) { return (k < split_src) ? k : k + gap; }

// ---- f32h_t shadows (ASE_F32H3): W * 2^e split into half hi / lo parts, packed [8 hi | 8 lo] per group of 8 consecutive elements of the
// contracted (contiguous) dimension - k for W_s, n for W_s^T; 4 bytes per element, leading dimensions in 4-byte units like the f32
// shadows they replace (written by ase_hip_refresh_shadow and ase_hip_apply_multi_v2, read by Mma<f32h_t> in gemm_nt_kernels.h) --------
// (saturating, like every other conversion into half storage: a weight beyond +-32 at the scale 2^11 must not become inf and then NaN
//  in every product; once per weight and step, free.  The A operand's split stays a plain cast in the kernel's loop: its inputs are
//  bounded by construction - observations clamped to +-5 at 2^12, see _gp_value)
__device__ __forceinline__ void split_half(float v, float scale, f16_t& hi, f16_t& lo) {
    const float s = __builtin_amdgcn_fmed3f(v * scale, -65504.f, 65504.f);
    hi = (f16_t)s;
    lo = (f16_t)(s - (float)hi);
}
__device__ __forceinline__ char* split_at(char* row, int col) { return row + (col >> 3) * 32 + (col & 7) * 2; }
__device__ __forceinline__ void store_split(char* row, int col, float v, float scale) {
    f16_t hi, lo;
    split_half(v, scale, hi, lo);
    char* g = split_at(row, col);
    *reinterpret_cast<f16_t*>(g) = hi;
    *reinterpret_cast<f16_t*>(g + 16) = lo;
}
// four consecutive elements from col % 4 == 0: 4 hi halves, 4 lo halves - half a group of 8 each
__device__ __forceinline__ void store_split4(char* row, int col, const float (&v)[4], float scale) {
    f16x4 h, l;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f16_t hh, ll;
        split_half(v[c], scale, hh, ll);
        h[c] = hh; l[c] = ll;
    }
    char* g = split_at(row, col);
    *reinterpret_cast<f16x4*>(g) = h;
    *reinterpret_cast<f16x4*>(g + 16) = l;
}

template <typename T> __device__ __forceinline__ void store_shadow4(T* p, const float (&w)[4]);
template <> __device__ __forceinline__ void store_shadow4<bf16_t>(bf16_t* p, const float (&w)[4]) {
    bf16x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (bf16_t)w[c];
    *reinterpret_cast<bf16x4*>(p) = v;
}
template <> __device__ __forceinline__ void store_shadow4<f16_t>(f16_t* p, const float (&w)[4]) {
    f16x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = from_f32<f16_t>(w[c]);
    *reinterpret_cast<f16x4*>(p) = v;
}
template <> __device__ __forceinline__ void store_shadow4<float>(float* p, const float (&w)[4]) {
    *reinterpret_cast<f32x4*>(p) = f32x4{w[0], w[1], w[2], w[3]};
}

// ---- sinks of the tile routine: a shadow pair takes element (n, kd) of W_s and element (kd, n) of W_s^T ---------------------------------
// plain storage type T, pitches in elements.  NULLABLE: either shadow may be absent (the single-layer ase_hip_refresh_shadow only)
template <typename T, bool NULLABLE = false> struct ShadowPair {
    T* Ws; int64_t ldws; T* Wts; int64_t ldwts;
    __device__ __forceinline__ void row(int n, int kd, float v) const {
        if (!NULLABLE || Ws) Ws[(int64_t)n * ldws + kd] = from_f32<T>(v);
    }
    __device__ __forceinline__ void col(int kd, int n, float v) const {
        if (!NULLABLE || Wts) Wts[(int64_t)kd * ldwts + n] = from_f32<T>(v);
    }
};
// the packed half split of W * scale (scale = 2^e), pitches in BYTES; either shadow may be absent wherever it is written
template <bool NULLABLE> struct ShadowPair<f32h_t, NULLABLE> {
    char* Ws; int64_t ldws; char* Wts; int64_t ldwts; float scale;
    __device__ __forceinline__ void row(int n, int kd, float v) const {
        if (Ws) store_split(Ws + (int64_t)n * ldws, kd, v, scale);
    }
    __device__ __forceinline__ void col(int kd, int n, float v) const {
        if (Wts) store_split(Wts + (int64_t)kd * ldwts, n, v, scale);
    }
};

// One 32 x 32 tile at (n0, k0) by 256 threads, thread (tx, ty) = (threadIdx.x & 31, threadIdx.x >> 5) of 32 x 8 (the caller's: the
// optimizer kernel shares them with its other path, which saves it a spilled register).  Phase 1: each thread's four (n, k) elements
// (rows of W coalesced) come from load(n, k) - out of range: zero - and go to tile[][] and to every sink's row-major shadow.  Barrier.
// Phase 2: the transposed shadows from the tile.  (A caller that walks several tiles puts its own barrier in front of each: the
// tile is still being read.)
template <int PITCH, typename Load, typename... Sinks>
__device__ __forceinline__ void shadow_tile32(float (*tile)[PITCH], int n0, int k0, int n_real, int k_real, int split_src, int gap,
                                              int tx, int ty, Load&& load, const Sinks&... sinks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + ty + 8 * i, k = k0 + tx;
        float v = 0.f;
        if (n < n_real && k < k_real) {
            v = load(n, k);
            (sinks.row(n, shadow_col(k, split_src, gap), v), ...);
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + ty + 8 * i, n = n0 + tx;
        if (k < k_real && n < n_real) (sinks.col(shadow_col(k, split_src, gap), n, tile[tx][ty + 8 * i]), ...);
    }
}
