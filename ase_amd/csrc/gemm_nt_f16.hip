// NT kernels of the storage type f16_t (see gemm_nt_kernels.h): the instantiations the library ships.
#include "gemm_nt_kernels.h"

int ase_nt::dispatch_nt_f16(const NTParams& p, hipStream_t s) { return dispatch_nt<f16_t>(p, s); }
int ase_nt::dispatch_nt_stacked_f16(const NTParams& p, hipStream_t s) { return dispatch_nt_stacked<f16_t>(p, s); }
