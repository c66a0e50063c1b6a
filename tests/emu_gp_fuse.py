"""EmuBackend with the fused epilogue duties of the penalty value path's matrix launches (HipBackend.gemm_nt's seed / twin / sq /
store arguments, ase_hip_gemm_nt_ex) in torch: the plain launch of tests/emu_backend.py, then each duty by the expression of the
helper launch it replaces (gp_seed, gather_multi's conversion, sqnorm)."""
import torch

from tests.emu_backend import EmuBackend, _dyn, _store


class FusedEmuBackend(EmuBackend):
    nt_fused_epilogue = True          # the capability engine_opts gp_fuse = 'auto' looks for
    x3 = False                        # (the engine switches it to 'f16' around the value path: x3_half_product)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.fused_launches = 0
        self.normalize_launches = 0
        self.split_shadow_writes = 0
        self.helper_launches = 0      # gp_seed / sqnorm / identity gather_multi: what gp_fuse removes

    def gemm_nt(self, A, B, Cm, M, N, K, seed=None, twin=None, sq=None, store=True, **kw):
        if seed is None and twin is None and sq is None:
            assert store
            return super().gemm_nt(A, B, Cm, M, N, K, **kw)
        assert kw.get('x3_exps') is not None and self.x3 == 'f16' and Cm.dtype == torch.float32
        assert kw.get('colsum') is None and (store or twin is not None)
        self.fused_launches += 1
        act = torch.zeros(M, N, dtype=torch.float32)
        super().gemm_nt(A, B, act, M, N, K, **kw)           # (mask_out describes the activation, not the seed)
        v = act
        if seed is not None:
            w, scale = seed
            wn = torch.zeros(N, dtype=torch.float32)
            wn[:w.numel()] = w
            v = scale * wn * (act > 0).float()               # gp_seed: scale * w[j] * [h > 0]
        if store:
            Cm[:M, :N] = v
        if twin is not None:
            twin[:M, :N] = _store(v, twin.dtype)
        if sq is not None:
            acc, slot, scale, dyn = sq
            acc[slot] += scale * _dyn(dyn) * (v.double() ** 2).sum()

    def rms_normalize_multi_twin(self, streams, D, M, means, stds, outs, outs32):
        for (src, idx, remap), mean, std, out, o32 in zip(streams, means, stds, outs, outs32):
            self.rms_normalize(src, D, idx, remap, M, mean, std, [out, o32])      # (each output rounds the same f32 value)

    def rms_normalize(self, *a, **kw):
        self.normalize_launches += 1
        return super().rms_normalize(*a, **kw)

    def apply_multi_split(self, desc, items, dtype, opt_state, acc, desc2, items2):
        self.apply_multi(desc, items, dtype, opt_state, acc)
        for it, it2 in zip(items, items2):        # (the emulator's value-path shadows are plain f32, see EmuBackend.refresh_shadow)
            if it2 is not None:
                self.split_shadow_writes += 1
                self.refresh_shadow(it[0], it2[0], it2[1], it[3], it[4], x3_exp=it2[2])

    def gp_seed(self, *a, **kw):
        self.helper_launches += 1
        return super().gp_seed(*a, **kw)

    def sqnorm(self, *a, **kw):
        self.helper_launches += 1
        return super().sqnorm(*a, **kw)

    def gather_multi(self, desc, items, idx, remap, M):
        if idx is None:
            self.helper_launches += 1
        return super().gather_multi(desc, items, idx, remap, M)
