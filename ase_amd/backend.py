"""Tensor-level wrapper over the C ABI: extracts pointers / leading dimensions from torch tensors
that live in HBM and enqueues the HIP kernels on torch's current stream.

PyTorch is used here only for device memory and streams.  All arithmetic of the update path
happens inside ``libase_hip.so``.  There is no CPU implementation in the product; the engine's
host logic is exercised on CPU by ``tests/emu_backend.py`` (test infrastructure with the same
method names).
"""
import ctypes as C

import torch

from . import lib as L


_HOSTFN = C.CFUNCTYPE(None, C.c_void_p)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ld(t):
    return 0 if t is None else int(t.stride(0))


def _code(dtype):
    if dtype == torch.bfloat16:
        return L.BF16
    if dtype == torch.float32:
        return L.F32
    if dtype == torch.float16:
        return L.F16
    raise L.AseHipError(f"unsupported storage dtype {dtype}")


class HipBackend:
    name = "hip"
    nt_fused_epilogue = True     # gemm_nt(seed=, twin=, sq=): UpdateEngine's engine_opts gp_fuse needs it
    nt_stack = True              # gemm_nt(stack=) and disc_head(gp_add=): UpdateEngine's engine_opts gp_stack needs them

    def __init__(self, device=None, x3=False):
        # x3: f32-stored GEMM operands are multiplied as three 16-bit MFMAs on a hi/lo split - True: bf16 parts (ASE_F32X3, any
        # operand range), 'f16': half parts of operands scaled by 2^ea / 2^eb (ASE_F32H3, gemm_nt only; the caller passes the
        # exponents of a launch as x3_exps=(ea, eb), see f32h_t in csrc/common.h)
        self.x3 = x3 if x3 == 'f16' else bool(x3)
        self._recording, self._host_keep, self._host_error = None, {}, None
        self.tn_workspace = True     # grouped weight gradients: partial tiles + reduce kernel (False: f32 atomics into G)
        if not torch.cuda.is_available():
            raise L.AseHipError("HipBackend needs a ROCm GPU (torch.cuda.is_available() is False); "
                                "the update path has no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.lib = L.get()
        self._head_scratch = torch.zeros(L.PPO_SCRATCH, dtype=torch.float64, device=self.device)   # (zeroed: it ends in a ticket word)
        self._head_scratch_ls = None          # the learned log-std's wider slabs (ASE_PPO_SCRATCH_LS), on first use

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def zero_(self, t):
        assert t.is_contiguous()
        L.check(self.lib.ase_hip_memset(_ptr(t), 0, t.numel() * t.element_size(), self._stream()), "memset")

    def copy_(self, dst, src):
        assert dst.is_contiguous() and src.is_contiguous() and dst.dtype == src.dtype and dst.numel() == src.numel()
        L.check(self.lib.ase_hip_memcpy(_ptr(dst), _ptr(src), dst.numel() * dst.element_size(), self._stream()), "memcpy")

    # ------------------------------------------------------------------ streams: fork / join, launch programs
    def mark(self):
        """Event at the current position of torch's current stream -> id (fork point / branch completion)."""
        ev = C.c_int(0)
        L.check(self.lib.ase_hip_mark(self._stream(), C.byref(ev)), "mark")
        return ev.value

    def wait(self, ev):
        """torch's current stream waits for the event."""
        L.check(self.lib.ase_hip_wait(self._stream(), int(ev)), "wait")

    def prog_create(self):
        p = C.c_void_p()
        L.check(self.lib.ase_hip_prog_create(C.byref(p)), "prog_create")
        return p

    def prog_begin(self, prog):
        L.check(self.lib.ase_hip_prog_begin(prog), "prog_begin")
        self._recording = prog.value
        self._host_keep.setdefault(prog.value, [])

    def prog_end(self, prog):
        self._recording = None
        L.check(self.lib.ase_hip_prog_end(prog), "prog_end")

    def host_call(self, fn):
        """A host-side operation at this position of the launch sequence (a collective, a torch op between kernels): run
        now, or - while a launch program records - on every replay (ase_hip_prog_host).  fn enqueues its own GPU work."""
        if self._recording is None:
            fn()
            return

        def trampoline(_arg, fn=fn):
            try:
                fn()
            except BaseException as e:           # an exception cannot cross the C frame: keep it for the caller of prog_launch
                self._host_error = e
        cb = _HOSTFN(trampoline)
        self._host_keep[self._recording].append(cb)          # the program calls through this object on every replay
        L.check(self.lib.ase_hip_prog_host(C.cast(cb, C.c_void_p), None), "prog_host")

    def prog_launch(self, prog):
        L.check(self.lib.ase_hip_prog_launch(prog), "prog_launch")
        if self._host_error is not None:
            e, self._host_error = self._host_error, None
            raise e

    def prog_size(self, prog):
        return self.lib.ase_hip_prog_size(prog)

    def prog_destroy(self, prog):
        self.lib.ase_hip_prog_destroy(prog)
        self._host_keep.pop(prog.value, None)

    def _gemm_code(self, dtype, exps=None):
        c = _code(dtype)
        if self.x3 and c == L.F32:
            if self.x3 == 'f16' and exps is not None:
                return L.F32H3 | (int(exps[0]) << 8) | (int(exps[1]) << 16)
            return L.F32X3
        return c

    # ------------------------------------------------------------------ GEMMs
    def gemm_nt(self, A, B, Cm, M, N, K, bias=None, aux=None, aux_mode=L.AUX_NONE, colsum=None, colsum_n=0,
                act=L.ACT_NONE, alpha=1.0, aux_split=0, aux_delta=0, mask_out=None, x3_exps=None, alpha_dev=None,
                seed=None, twin=None, sq=None, store=True, stack=None):
        """stack = (split, aux2, alpha2, alpha_dev2) (nt_stack; ase_hip_gemm_nt_stacked): rows [split, M) are a second row block with
        duties of its own - no bias, activation or mask_out, scale alpha2 / alpha_dev2, the optional bit mask aux2 [M - split, N / 32]
        read at row m - split; bias, act, mask_out (its first `split` rows), alpha and alpha_dev then belong to rows [0, split) alone.
        seed / twin / sq (nt_fused_epilogue; ASE_F32H3 launches only - ase_hip_gemm_nt_ex): duties of the launch's epilogue that
        were launches of their own.  seed = (w f32[n], scale): store scale * w[col] * [act(z) > 0] instead of the activation (gp_seed);
        twin = a 16-bit tensor that receives the stored values once more (the conversion of gather_multi; store=False with a twin: Cm
        names the shape only and is NOT written);
        sq = (acc, slot, scale, dyn): acc[slot] += scale * dyn's factor * sum of the stored values' squares (sqnorm).
        alpha_dev (all `*_dev` / `dyn` arguments of this class): a scale RECORD on the device, f32 {factor, overflow count} - an
        entry of the dynamic loss scale's table (UpdateEngine.scale_tab: S, 1 / S, 1 / S^2, 1).  The launch multiplies its scale by the
        factor when it RUNS and adds to the count when an element it stored overflowed (include/ase_hip.h, ABI 7)."""
        dt = self._gemm_code(A.dtype, x3_exps)
        assert B.dtype == A.dtype
        if aux_mode == L.AUX_RELU_BITS:
            assert aux.dtype == torch.int32
        else:
            assert aux is None or aux.dtype == A.dtype
        # twin output: the ReLU bit matrix (int32 words), or for the smooth activations the pre-activation in the storage type
        assert mask_out is None or mask_out.dtype == (A.dtype if act >= L.ACT_SILU else torch.int32)
        if seed is not None or twin is not None or sq is not None:
            assert (dt & 0xFF) == L.F32H3, "seed / twin / sq belong to the half-split f32 launches (x3 = 'f16', x3_exps)"
            assert Cm.dtype == torch.float32 and (store or twin is not None)
            sw, ss = seed if seed is not None else (None, 0.0)
            acc, slot, sscale, dyn = sq if sq is not None else (None, 0, 0.0, None)
            assert acc is None or acc.dtype == torch.float64
            L.check(self.lib.ase_hip_gemm_nt_ex(_ptr(A), _ld(A), _ptr(B), _ld(B), _ptr(Cm) if store else None, _ld(Cm), _ptr(bias), _ptr(aux),
                                                _ld(aux), int(aux_split), int(aux_delta), _ptr(colsum), int(colsum_n),
                                                _ptr(mask_out), _ld(mask_out), M, N, K, act, aux_mode, 0,
                                                float(alpha), _ptr(alpha_dev), dt,
                                                _ptr(sw), 0 if sw is None else sw.numel(), float(ss),
                                                _ptr(twin), _ld(twin), 0 if twin is None else _code(twin.dtype),
                                                None if acc is None else C.c_void_p(acc.data_ptr() + 8 * int(slot)), float(sscale),
                                                _ptr(dyn), self._stream()), "gemm_nt_ex")
            return
        out_f32 = int(Cm.dtype == torch.float32 and A.dtype != torch.float32)
        if stack is not None:
            split, aux2, alpha2, alpha_dev2 = stack
            assert aux is None and aux_mode == L.AUX_NONE and colsum is None, "a stacked launch takes its mask operand in stack=(...)"
            assert aux2 is None or aux2.dtype == torch.int32
            L.check(self.lib.ase_hip_gemm_nt_stacked(_ptr(A), _ld(A), _ptr(B), _ld(B), _ptr(Cm), _ld(Cm), _ptr(bias), _ptr(aux2),
                                                     _ld(aux2), int(split), int(split), None, 0, _ptr(mask_out), _ld(mask_out),
                                                     M, N, K, act, L.AUX_NONE if aux2 is None else L.AUX_RELU_BITS, out_f32,
                                                     float(alpha), _ptr(alpha_dev), int(split), float(alpha2), _ptr(alpha_dev2), dt,
                                                     self._stream()), "gemm_nt_stacked")
            return
        L.check(self.lib.ase_hip_gemm_nt(_ptr(A), _ld(A), _ptr(B), _ld(B), _ptr(Cm), _ld(Cm), _ptr(bias), _ptr(aux),
                                         _ld(aux), int(aux_split), int(aux_delta), _ptr(colsum), int(colsum_n),
                                         _ptr(mask_out), _ld(mask_out), M, N, K, act, aux_mode, out_f32,
                                         float(alpha), _ptr(alpha_dev), dt, self._stream()), "gemm_nt")

    def gemm_tn(self, A, B, G, M, N, K, n_real, k_real, split_src, split_dst, alpha=1.0, gbias=None, bias_rows=0, alpha_dev=None):
        L.check(self.lib.ase_hip_gemm_tn(_ptr(A), _ld(A), _ptr(B), _ld(B), _ptr(G), _ptr(gbias), int(bias_rows), M, N, K,
                                         n_real, k_real,
                                         split_src, split_dst, float(alpha), _ptr(alpha_dev), self._gemm_code(A.dtype), self._stream()),
                "gemm_tn")

    # grouped weight gradients: one launch for every (eligible) dense layer of a step
    def grouped_tn_ok(self, dtype, M, n_real, K, bias_rows):
        """Problems the phased bf16 kernel takes: whole 64-row K-tiles.  Narrow outputs (heads, style MLP: N or K <= 64)
        waste most of a 256 x 256 tile's MFMAs, but a work item costs its HBM traffic either way: measured (scripts/lab,
        LAB_TNG_N) the six narrow problems of a step add 67 us to the grouped launch against 156 us as seven launches of the
        128 x 128 kernel."""
        return dtype in (torch.bfloat16, torch.float16) and M % 64 == 0 and bias_rows % 64 == 0

    def make_tn_plan(self, problems, target_wg=0, alpha_dev=None):
        """problems: [(A, B, G, gbias|None, bias_rows, M, N, K, n_real, k_real, split_src, split_dst, alpha)] -> plan
        (device tables + the tensors they point to, kept alive)."""
        import struct
        n = len(problems)
        tab = (C.c_int64 * (16 * n))()
        for i, (A, B, G, gb, br, M, N, K, nr, kr, ss, sd, alpha) in enumerate(problems):
            assert A.dtype in (torch.bfloat16, torch.float16) and B.dtype == A.dtype and G.dtype == torch.float32
            row = [A.data_ptr(), _ld(A), B.data_ptr(), _ld(B), G.data_ptr(), 0 if gb is None else gb.data_ptr(), int(br),
                   M, N, K, nr, kr, ss, sd, struct.unpack('<i', struct.pack('<f', float(alpha)))[0], 0]
            for j, v in enumerate(row):
                tab[16 * i + j] = int(v)
        max_work = 8192
        work = (C.c_int32 * (4 * max_work))()
        red = (C.c_int32 * (4 * max_work))()
        n_work, n_red = C.c_int(0), C.c_int(0)
        L.check(self.lib.ase_hip_gemm_tn_grouped_plan(tab, n, int(target_wg), work, max_work, C.byref(n_work), red, max_work,
                                                      C.byref(n_red)), "gemm_tn_grouped_plan")
        nw, nr = n_work.value, n_red.value
        dev_tab = torch.tensor(list(tab), dtype=torch.int64, device=self.device)
        dev_work = torch.tensor(list(work[:4 * nw]), dtype=torch.int32, device=self.device)
        dev_red = torch.tensor(list(red[:4 * nr]), dtype=torch.int32, device=self.device)
        # partial-sum workspace of this launch (plans of different branches run side by side: one each)
        ws = torch.empty(nw * L.TN_SLAB, dtype=torch.float32, device=self.device) if self.tn_workspace else None
        return {'problems': dev_tab, 'work': dev_work, 'n_work': nw, 'red': dev_red, 'n_red': nr, 'ws': ws, 'keep': problems,
                'dtype': _code(problems[0][0].dtype), 'alpha_dev': alpha_dev}

    def gemm_tn_grouped(self, plan):
        L.check(self.lib.ase_hip_gemm_tn_grouped(_ptr(plan['problems']), _ptr(plan['work']), plan['n_work'], _ptr(plan['red']),
                                                 plan['n_red'], _ptr(plan['ws']), _ptr(plan.get('alpha_dev')), plan['dtype'],
                                                 self._stream()),
                "gemm_tn_grouped")

    def refresh_shadow(self, W, Ws, Wts, split_src, split_dst, x3_exp=None):
        """x3_exp (f32 shadows only): write them in the packed half-split format of ASE_F32H3 - W * 2^x3_exp as [8 hi | 8 lo] halves
        per group of 8 elements, the B operand of gemm_nt(..., x3_exps=(ea, x3_exp)) under x3 = 'f16'."""
        n, k = W.shape
        ref = Ws if Ws is not None else Wts
        code = _code(ref.dtype)
        if x3_exp is not None:
            assert ref.dtype == torch.float32
            code = L.F32H3 | (int(x3_exp) << 16)
        L.check(self.lib.ase_hip_refresh_shadow(_ptr(W), n, k, _ptr(Ws), _ld(Ws), _ptr(Wts), _ld(Wts), split_src,
                                                split_dst, code, self._stream()), "refresh_shadow")

    def refresh_shadow_multi(self, desc, items, dtype):
        """desc: device int64 [n, 12] pointer table (see ase_hip.h); items: the same tensors (kept alive by the caller)."""
        L.check(self.lib.ase_hip_refresh_shadow_multi(_ptr(desc), desc.shape[0], _code(dtype), self._stream()),
                "refresh_shadow_multi")

    def apply_multi(self, desc, items, dtype, opt_state, acc):
        """Fused optimizer step + shadow refresh of every layer (desc: device int64 [n, 24], see ase_hip.h)."""
        L.check(self.lib.ase_hip_apply_multi(_ptr(desc), desc.shape[0], _ptr(opt_state), _ptr(acc), _code(dtype),
                                             self._stream()), "apply_multi")

    def apply_multi_split(self, desc, items, dtype, opt_state, acc, desc2, items2):
        """apply_multi that also writes a second, half-split (ASE_F32H3) shadow pair per layer (desc2: device int64 [n, 8] rows
        {Ws3, ldws3, Wts3, ldwts3, exponent, 0, 0, 0}, zeros = none; see ase_hip.h; items2: the same tensors as (Ws3, Wts3, exponent) or None per row, kept alive by the caller)."""
        assert desc2.shape == (desc.shape[0], 8) and desc2.is_contiguous()
        L.check(self.lib.ase_hip_apply_multi_v2(_ptr(desc), desc.shape[0], _ptr(desc2), _ptr(opt_state), _ptr(acc), _code(dtype),
                                                self._stream()), "apply_multi_v2")

    def gather_multi(self, desc, items, idx, remap, M):
        L.check(self.lib.ase_hip_gather_multi(_ptr(desc), desc.shape[0], _ptr(idx), remap[0], remap[1], M,
                                              self._stream()), "gather_multi")

    # ------------------------------------------------------------------ observation side (N2)
    def build_amp_obs(self, root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos, dof_offsets,
                      local_root_obs, root_height_obs, hist, shift=True):
        """One AMP-observation frame per env pushed into hist [N, S, F] (env/tasks/humanoid_amp.py:248-316)."""
        n, S, F = hist.shape
        offs = (C.c_int32 * len(dof_offsets))(*[int(x) for x in dof_offsets])
        for t in (root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos, hist):
            assert t.dtype == torch.float32 and t.is_contiguous()
        L.check(self.lib.ase_hip_build_amp_obs(_ptr(root_pos), _ptr(root_rot), _ptr(root_vel), _ptr(root_ang_vel), _ptr(dof_pos),
                                               _ptr(dof_vel), _ptr(key_body_pos), n, dof_pos.shape[1], key_body_pos.shape[1], offs,
                                               len(dof_offsets) - 1, int(local_root_obs), int(root_height_obs), _ptr(hist), S,
                                               int(shift), self._stream()), "build_amp_obs")

    def motion_state(self, clips, motion_ids, times):
        """MotionLib.get_motion_state (utils/motion_lib.py:122-172) on device clip tensors.  clips: dict with gts, grs, lrs,
        grvs, gravs, dvs (f32), lengths, dt (f32), num_frames, length_starts (int32) on this device and the python lists
        dof_body_ids, dof_offsets, key_body_ids.  Returns (root_pos, root_rot, dof_pos, root_vel, root_ang_vel, dof_vel, key_pos)."""
        n, B = motion_ids.shape[0], clips['gts'].shape[1]
        D, J, K = clips['dof_offsets'][-1], len(clips['dof_body_ids']), len(clips['key_body_ids'])
        ia = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        out = (f(n, 3), f(n, 4), f(n, D), f(n, 3), f(n, 3), f(n, D), f(n, K, 3))
        assert motion_ids.dtype == torch.int32 and times.dtype == torch.float32
        L.check(self.lib.ase_hip_motion_state(_ptr(clips['gts']), _ptr(clips['grs']), _ptr(clips['lrs']), _ptr(clips['grvs']),
                                              _ptr(clips['gravs']), _ptr(clips['dvs']), B, _ptr(clips['lengths']),
                                              _ptr(clips['num_frames']), _ptr(clips['dt']), _ptr(clips['length_starts']),
                                              _ptr(motion_ids), _ptr(times), n, ia(clips['dof_body_ids']), ia(clips['dof_offsets']), J,
                                              ia(clips['key_body_ids']), K, *[_ptr(o) for o in out], self._stream()), "motion_state")
        return out

    def clip_frames(self, rotation, root_translation, root_velocity, root_angular_velocity, local_translation, parent_indices,
                    clip_first, clip_num_frames, clip_fps, frame_clip, dof_body_ids, dof_offsets, out=None):
        """The frame arrays of motion_state from the raw contents of clip files (MotionLib._load_motions +
        _compute_motion_dof_vels, utils/motion_lib.py:75-80,174-236,279-294; operands: see ase_hip_clip_frames), one launch.
        rotation [T, B, 4], root_translation / root_velocity / root_angular_velocity [T, 3], clip_fps [C]: f64;
        local_translation [C, B, 3]: f32; clip_first, clip_num_frames [C], frame_clip [T]: int32; parent_indices, dof_body_ids,
        dof_offsets: python lists.  Returns (gts, grs, lrs, grvs, gravs, dvs), f32 (out: the six tensors to write instead)."""
        T, B = rotation.shape[0], rotation.shape[1]
        Cn, J, D = clip_first.numel(), len(dof_body_ids), int(dof_offsets[-1])
        for t, dt, shape in ((rotation, torch.float64, (T, B, 4)), (root_translation, torch.float64, (T, 3)),
                             (root_velocity, torch.float64, (T, 3)), (root_angular_velocity, torch.float64, (T, 3)),
                             (local_translation, torch.float32, (Cn, B, 3)), (clip_first, torch.int32, (Cn,)),
                             (clip_num_frames, torch.int32, (Cn,)), (clip_fps, torch.float64, (Cn,)), (frame_clip, torch.int32, (T,))):
            assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device.type == self.device.type, \
                f"clip_frames: operand {tuple(t.shape)} {t.dtype}, expected {shape} {dt} on {self.device}"
        assert len(parent_indices) == B and len(dof_offsets) == J + 1
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        if out is None:
            out = (f(T, B, 3), f(T, B, 4), f(T, B, 4), f(T, 3), f(T, 3), f(T, D))
        for o, shape in zip(out, ((T, B, 3), (T, B, 4), (T, B, 4), (T, 3), (T, 3), (T, D))):
            assert o.dtype == torch.float32 and tuple(o.shape) == shape and o.is_contiguous() and o.device.type == self.device.type
        ia = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])
        L.check(self.lib.ase_hip_clip_frames(_ptr(rotation), _ptr(root_translation), _ptr(root_velocity), _ptr(root_angular_velocity),
                                             _ptr(local_translation), ia(parent_indices), B, _ptr(clip_first), _ptr(clip_num_frames),
                                             _ptr(clip_fps), _ptr(frame_clip), Cn, T, ia(dof_body_ids), ia(dof_offsets), J,
                                             *[_ptr(o) for o in out], self._stream()), "clip_frames")
        return tuple(out)

    # ------------------------------------------------------------------ retargeting (N16; operands: see ase_hip_retarget_*)
    def _rt_check(self, name, *specs):
        for t, dt, shape in specs:
            assert t.dtype == dt and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device.type == self.device.type, \
                f"{name}: operand {tuple(t.shape)} {t.dtype}, expected {tuple(shape)} {dt} on {self.device}"

    def _rt_out(self, name, out, *specs):
        if out is None:
            return tuple(torch.empty(*shape, dtype=dt, device=self.device) for dt, shape in specs)
        out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        self._rt_check(name, *[(o, dt, shape) for o, (dt, shape) in zip(out, specs)])
        return out

    def retarget_fk(self, rotation, mode, tree, clip_first, clip_num_frames, src_first, frame_clip, out=None):
        """Global rotations of a tree for the frames the clip tables select -> f64 [T, B, 4].  rotation f64 [Tsrc, B, 4]; mode 0
        local rotations, 1 global as stored, 2 global through local form; tree int32 [B, ld]; the four tables int32."""
        f64, i32 = torch.float64, torch.int32
        Ts, B, T, Cn = rotation.shape[0], rotation.shape[1], frame_clip.numel(), clip_first.numel()
        self._rt_check('retarget_fk', (rotation, f64, (Ts, B, 4)), (tree, i32, (B, tree.shape[1])), (clip_first, i32, (Cn,)),
                       (clip_num_frames, i32, (Cn,)), (src_first, i32, (Cn,)), (frame_clip, i32, (T,)))
        out, = self._rt_out('retarget_fk', out, (f64, (T, B, 4)))
        L.check(self.lib.ase_hip_retarget_fk(_ptr(rotation), int(mode), _ptr(tree), tree.shape[1], B, _ptr(clip_first),
                                             _ptr(clip_num_frames), _ptr(src_first), _ptr(frame_clip), Cn, T, Ts, _ptr(out),
                                             self._stream()), "retarget_fk")
        return out

    def retarget_chain(self, src_global, rs_body, rs_parent, rt_src, rt_tree, params, out=None):
        """Source global rotations f64 [T, Bs, 4] -> global rotations on the reduced target tree, f64 [T, M, 4]."""
        f64, i32 = torch.float64, torch.int32
        T, Bs, M = src_global.shape[0], src_global.shape[1], rs_body.numel()
        self._rt_check('retarget_chain', (src_global, f64, (T, Bs, 4)), (rs_body, i32, (M,)), (rs_parent, i32, (M,)),
                       (rt_src, i32, (M,)), (rt_tree, i32, (M, rt_tree.shape[1])), (params, f64, (12,)))
        out, = self._rt_out('retarget_chain', out, (f64, (T, M, 4)))
        L.check(self.lib.ase_hip_retarget_chain(_ptr(src_global), Bs, _ptr(rs_body), _ptr(rs_parent), _ptr(rt_src), _ptr(rt_tree),
                                                rt_tree.shape[1], M, _ptr(params), T, _ptr(out), self._stream()), "retarget_chain")
        return out

    def retarget_pose(self, state_global, tpose_global, target_global, root_translation, params, rt_body, ancestor, parent_indices,
                      clip_first, clip_num_frames, src_first, frame_clip, out=None):
        """-> (local rotations on the target tree f64 [T, Bt, 4], root translation f64 [T, 3])."""
        f64, i32 = torch.float64, torch.int32
        T, M, Bt, Ts, Cn = state_global.shape[0], state_global.shape[1], ancestor.numel(), root_translation.shape[0], clip_first.numel()
        self._rt_check('retarget_pose', (state_global, f64, (T, M, 4)), (tpose_global, f64, (M, 4)), (target_global, f64, (Bt, 4)),
                       (root_translation, f64, (Ts, 3)), (params, f64, (12,)), (rt_body, i32, (M,)), (ancestor, i32, (Bt,)),
                       (parent_indices, i32, (Bt,)), (clip_first, i32, (Cn,)), (clip_num_frames, i32, (Cn,)), (src_first, i32, (Cn,)),
                       (frame_clip, i32, (T,)))
        out = self._rt_out('retarget_pose', out, (f64, (T, Bt, 4)), (f64, (T, 3)))
        L.check(self.lib.ase_hip_retarget_pose(_ptr(state_global), _ptr(tpose_global), _ptr(target_global), _ptr(root_translation),
                                               _ptr(params), _ptr(rt_body), _ptr(ancestor), _ptr(parent_indices), M, Bt,
                                               _ptr(clip_first), _ptr(clip_num_frames), _ptr(src_first), _ptr(frame_clip), Cn, T, Ts,
                                               _ptr(out[0]), _ptr(out[1]), self._stream()), "retarget_pose")
        return out

    def retarget_hinge(self, local_rotation, root_translation, local_translation, tree, roles, out=None):
        """project_joints from the roles table int32 [B, 6] -> local rotations f64 [T, B, 4]."""
        f64, i32 = torch.float64, torch.int32
        T, B = local_rotation.shape[0], local_rotation.shape[1]
        self._rt_check('retarget_hinge', (local_rotation, f64, (T, B, 4)), (root_translation, f64, (T, 3)),
                       (local_translation, torch.float32, (B, 3)), (tree, i32, (B, tree.shape[1])), (roles, i32, (B, 6)))
        out, = self._rt_out('retarget_hinge', out, (f64, (T, B, 4)))
        L.check(self.lib.ase_hip_retarget_hinge(_ptr(local_rotation), _ptr(root_translation), _ptr(local_translation), _ptr(tree),
                                                tree.shape[1], _ptr(roles), B, T, _ptr(out), self._stream()), "retarget_hinge")
        return out

    def retarget_ground(self, local_rotation, root_translation, local_translation, tree, clip_first, clip_num_frames, out=None):
        """-> per clip the minimum of global z over its frames and bodies, f64 [C]."""
        f64, i32 = torch.float64, torch.int32
        T, B, Cn = local_rotation.shape[0], local_rotation.shape[1], clip_first.numel()
        self._rt_check('retarget_ground', (local_rotation, f64, (T, B, 4)), (root_translation, f64, (T, 3)),
                       (local_translation, torch.float32, (B, 3)), (tree, i32, (B, tree.shape[1])), (clip_first, i32, (Cn,)),
                       (clip_num_frames, i32, (Cn,)))
        out, = self._rt_out('retarget_ground', out, (f64, (Cn,)))
        L.check(self.lib.ase_hip_retarget_ground(_ptr(local_rotation), _ptr(root_translation), _ptr(local_translation), _ptr(tree),
                                                 tree.shape[1], B, _ptr(clip_first), _ptr(clip_num_frames), Cn, T, _ptr(out),
                                                 self._stream()), "retarget_ground")
        return out

    def retarget_finish(self, local_rotation, root_translation, min_z, params, local_translation, tree, frame_clip, out=None):
        """-> (global rotation f64 [T, B, 4], global translation f64 [T, B, 3], rotation f32 [T, B, 4], root translation f32 [T, 3])
        of the grounded motion."""
        f64, f32, i32 = torch.float64, torch.float32, torch.int32
        T, B, Cn = local_rotation.shape[0], local_rotation.shape[1], min_z.numel()
        self._rt_check('retarget_finish', (local_rotation, f64, (T, B, 4)), (root_translation, f64, (T, 3)), (min_z, f64, (Cn,)),
                       (params, f64, (12,)), (local_translation, f32, (B, 3)), (tree, i32, (B, tree.shape[1])), (frame_clip, i32, (T,)))
        out = self._rt_out('retarget_finish', out, (f64, (T, B, 4)), (f64, (T, B, 3)), (f32, (T, B, 4)), (f32, (T, 3)))
        L.check(self.lib.ase_hip_retarget_finish(_ptr(local_rotation), _ptr(root_translation), _ptr(min_z), _ptr(params),
                                                 _ptr(local_translation), _ptr(tree), tree.shape[1], B, _ptr(frame_clip), Cn, T,
                                                 *[_ptr(o) for o in out], self._stream()), "retarget_finish")
        return out

    def retarget_velocity(self, global_rotation, global_translation, clip_first, clip_num_frames, clip_fps, frame_clip, out=None):
        """-> (global velocity, global angular velocity), f32 [T, B, 3]."""
        f64, f32, i32 = torch.float64, torch.float32, torch.int32
        T, B, Cn = global_rotation.shape[0], global_rotation.shape[1], clip_first.numel()
        self._rt_check('retarget_velocity', (global_rotation, f64, (T, B, 4)), (global_translation, f64, (T, B, 3)),
                       (clip_first, i32, (Cn,)), (clip_num_frames, i32, (Cn,)), (clip_fps, f64, (Cn,)), (frame_clip, i32, (T,)))
        out = self._rt_out('retarget_velocity', out, (f32, (T, B, 3)), (f32, (T, B, 3)))
        L.check(self.lib.ase_hip_retarget_velocity(_ptr(global_rotation), _ptr(global_translation), B, _ptr(clip_first),
                                                   _ptr(clip_num_frames), _ptr(clip_fps), _ptr(frame_clip), Cn, T, _ptr(out[0]),
                                                   _ptr(out[1]), self._stream()), "retarget_velocity")
        return out

    # ------------------------------------------------------------------ environment side (N5)
    @staticmethod
    def _f32c(*ts):
        for t in ts:
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), "state tensors are contiguous f32"

    @staticmethod
    def _rows(obs, env_ids):
        assert obs.dtype == torch.float32 and obs.dim() == 2 and obs.stride(1) == 1, "obs: f32 [rows, columns], unit column stride"
        if env_ids is None:
            return None, 0
        assert env_ids.dtype == torch.int32 and env_ids.is_contiguous() and env_ids.dim() == 1
        return env_ids, env_ids.numel()

    def humanoid_obs_max(self, body_pos, body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs, obs, col_offset=0,
                         env_ids=None):
        """compute_humanoid_observations_max (env/tasks/humanoid.py:592-636) into columns col_offset.. of obs [n_envs, >=]; with
        env_ids (int32) only those environments are computed and only their rows written."""
        n, B = body_pos.shape[0], body_pos.shape[1]
        self._f32c(body_pos, body_rot, body_vel, body_ang_vel)
        ids, n_ids = self._rows(obs, env_ids)
        if env_ids is not None and n_ids == 0:                # an empty tensor has a null pointer, which the entry reads as "every row"
            return
        assert obs.shape[0] >= n and body_rot.shape == (n, B, 4) and body_vel.shape == body_ang_vel.shape == body_pos.shape == (n, B, 3)
        L.check(self.lib.ase_hip_humanoid_obs_max(_ptr(body_pos), _ptr(body_rot), _ptr(body_vel), _ptr(body_ang_vel), n, B,
                                                  int(local_root_obs), int(root_height_obs), _ptr(ids), n_ids, _ptr(obs),
                                                  obs.stride(0), int(col_offset), self._stream()), "humanoid_obs_max")

    def humanoid_reset(self, progress_buf, contact_forces, body_pos, termination_heights, contact_body_ids, max_episode_length,
                       enable_early_termination, reset, terminated, tar_contact_forces=None, strike_body_ids=None):
        """compute_humanoid_reset (env/tasks/humanoid.py:645-672); with tar_contact_forces + strike_body_ids the strike form
        (env/tasks/humanoid_strike.py:255-297).  The body id lists are python lists; reset / terminated: int64 [n_envs]."""
        n, B = body_pos.shape[0], body_pos.shape[1]
        self._f32c(contact_forces, body_pos, termination_heights, tar_contact_forces)
        for t in (progress_buf, reset, terminated):
            assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n
        assert contact_forces.shape == body_pos.shape == (n, B, 3) and termination_heights.numel() == B
        assert tar_contact_forces is None or tar_contact_forces.shape == (n, 3)
        ia = lambda xs: None if xs is None else (C.c_int32 * len(xs))(*[int(x) for x in xs])
        L.check(self.lib.ase_hip_humanoid_reset(_ptr(progress_buf), _ptr(contact_forces), _ptr(body_pos), _ptr(termination_heights),
                                                ia(contact_body_ids), len(contact_body_ids), _ptr(tar_contact_forces),
                                                ia(strike_body_ids), 0 if strike_body_ids is None else len(strike_body_ids), n, B,
                                                float(max_episode_length), int(enable_early_termination), _ptr(reset),
                                                _ptr(terminated), self._stream()), "humanoid_reset")

    def task_obs(self, kind, obs, col_offset=0, env_ids=None, root_states=None, tar_a=None, tar_b=None, tar_speed=None,
                 tar_states=None):
        """Task observation of kind L.TASK_* (5 / 2 / 3 / 15 columns, see ase_hip.h) into columns col_offset.. of obs."""
        self._f32c(root_states, tar_a, tar_b, tar_speed, tar_states)
        ids, n_ids = self._rows(obs, env_ids)
        if env_ids is not None and n_ids == 0:                # as in humanoid_obs_max: an empty list writes nothing
            return
        n = obs.shape[0] if root_states is None else root_states.shape[0]
        for t, cols in ((root_states, 13), (tar_a, 3 if kind == L.TASK_REACH else 2), (tar_b, 2), (tar_speed, 1), (tar_states, 13)):
            assert t is None or t.numel() == n * cols, "task_obs: operand shape"
        L.check(self.lib.ase_hip_task_obs(int(kind), _ptr(root_states), _ptr(tar_a), _ptr(tar_b), _ptr(tar_speed), _ptr(tar_states), n,
                                          _ptr(ids), n_ids, _ptr(obs), obs.stride(0), int(col_offset), self._stream()), "task_obs")

    def task_reward(self, kind, reward, root_states=None, prev_root_pos=None, tar_a=None, tar_b=None, tar_speed=None,
                    tar_states=None, body_pos=None, body_id=0, dt=0.0):
        """Task reward of kind L.TASK_* into reward [n_envs]; tar_speed: tensor [n] (heading) or python float (location)."""
        speed_t = tar_speed if torch.is_tensor(tar_speed) else None
        self._f32c(root_states, prev_root_pos, tar_a, tar_b, speed_t, tar_states, body_pos, reward)
        n = reward.numel()
        for t, cols in ((root_states, 13), (prev_root_pos, 3), (tar_a, 3 if kind == L.TASK_REACH else 2), (tar_b, 2), (speed_t, 1),
                        (tar_states, 13)):
            assert t is None or t.numel() == n * cols, "task_reward: operand shape"
        assert body_pos is None or (body_pos.dim() == 3 and body_pos.shape[0] == n and body_pos.shape[2] == 3)
        L.check(self.lib.ase_hip_task_reward(int(kind), _ptr(root_states), _ptr(prev_root_pos), _ptr(tar_a), _ptr(tar_b), _ptr(speed_t),
                                             0.0 if speed_t is not None or tar_speed is None else float(tar_speed), _ptr(tar_states),
                                             _ptr(body_pos), 0 if body_pos is None else body_pos.shape[1], int(body_id), float(dt), n,
                                             _ptr(reward), self._stream()), "task_reward")

    # ------------------------------------------------------------------ target resets of the tasks (N8)
    def task_reset(self, kind, progress_buf=None, change_steps=None, root_states=None, tar_a=None, tar_b=None, tar_speed=None,
                   tar_states=None, env_ids=None, u=None, steps=None, rng_state=None, advance=True, steps_low=0, steps_high=0,
                   tar_speed_min=0.0, tar_speed_max=0.0, tar_dist_min=0.0, tar_dist_max=0.0, tar_height_min=0.0, tar_height_max=0.0,
                   near_dist=0.0, near_prob=0.0, enable_rand_heading=True):
        """_reset_task / _reset_target / _update_task of kind L.TASK_* in one launch (operands: see ase_hip_task_reset).
        env_ids (int32, distinct) names the rows, None: every environment with progress_buf >= change_steps.  The draws are
        either passed in (u f32 [n_ids, L.TASK_RESET_DRAWS[kind]], steps int64 [n_ids]) or made on the device from rng_state
        (int64 [2] = seed | offset, advanced by one unless advance is false).  tar_a / tar_b / tar_speed / tar_states and
        change_steps are written in place; root_states / tar_states [N, 13] may be strided views with unit column stride.
        The strike task reads root_states when the launch runs: call it after the actor reset."""
        self._f32c(tar_a, tar_b, tar_speed, u)
        n = next(t for t in (progress_buf, root_states, tar_states) if t is not None).shape[0]
        for t in (root_states, tar_states):
            assert t is None or (t.dtype == torch.float32 and t.shape == (n, 13) and t.stride(1) == 1), "[n, 13] f32, unit column stride"
        for t in (progress_buf, change_steps, steps):
            assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 1), "int64 vectors"
        for t, cols in ((progress_buf, 1), (change_steps, 1), (tar_a, 3 if kind == L.TASK_REACH else 2), (tar_b, 2), (tar_speed, 1)):
            assert t is None or t.numel() == n * cols, "task_reset: operand shape"
        n_ids = 0
        if env_ids is not None:
            assert env_ids.dtype == torch.int32 and env_ids.is_contiguous() and env_ids.dim() == 1
            n_ids = env_ids.numel()
        assert u is None or (0 <= kind < 4 and u.shape == (n_ids, L.TASK_RESET_DRAWS[kind])), "u: [n_ids, draws of the kind]"
        assert steps is None or steps.numel() == n_ids
        assert rng_state is None or (rng_state.dtype == torch.int64 and rng_state.numel() == 2 and rng_state.is_contiguous())
        L.check(self.lib.ase_hip_task_reset(int(kind), _ptr(env_ids), n_ids, _ptr(u), _ptr(steps), _ptr(rng_state), int(advance),
                                            _ptr(progress_buf), _ptr(change_steps), int(steps_low), int(steps_high),
                                            _ptr(root_states), _ld(root_states), _ptr(tar_a), _ptr(tar_b), _ptr(tar_speed),
                                            _ptr(tar_states), _ld(tar_states), float(tar_speed_min), float(tar_speed_max),
                                            float(tar_dist_min), float(tar_dist_max), float(tar_height_min), float(tar_height_max),
                                            float(near_dist), float(near_prob), int(enable_rand_heading), n, self._stream()),
                "task_reset")

    # ------------------------------------------------------------------ projectile launches of the perturbation task (N15)
    def proj_launch(self, root_states, body_pos, body_vel, proj_states, progress_buf=None, timesteps=None, slot=-1, env_ids=None,
                    u=None, eps=None, rng_state=None, advance=True, tar_body=1, dist_min=4.0, dist_max=5.0, h_min=0.25, h_max=2.0,
                    speed_min=30.0, speed_max=40.0, noise=0.1, slot_out=None, ids_out=None, draws_out=None):
        """HumanoidPerturb._update_proj in one launch (operands: see ase_hip_proj_launch).  root_states f32 [n, 13], body_pos /
        body_vel f32 [n, B, 3] and proj_states f32 [n, K, 13] are read / written in place and may be strided views with unit
        stride in the last dimension.  slot -1: due mode on progress_buf[0] (int64 [n]) and timesteps (int32 [K']); slot >= 0:
        that projectile, for every environment or for env_ids (int32, distinct).  The draws are passed in (u f32 [rows, 4], eps
        f32 [rows, 3]) or made on the device from rng_state (int64 [2] = seed | offset, advanced by one unless advance is false).
        slot_out int32 [1], ids_out int32 [n], draws_out f32 [n, 7] are optional exports.  The entry takes raw addresses: every
        tensor lives on the backend's device.  Recordable in a launch program."""
        f32 = torch.float32
        tensors = dict(root_states=root_states, body_pos=body_pos, body_vel=body_vel, proj_states=proj_states, progress_buf=progress_buf,
                       timesteps=timesteps, env_ids=env_ids, u=u, eps=eps, rng_state=rng_state, slot_out=slot_out, ids_out=ids_out,
                       draws_out=draws_out)
        for who, t in tensors.items():
            assert t is None or self._here(t), f"proj_launch: {who} must be a tensor on {self.device}, not {t.device}"
        assert root_states.dtype == f32 and root_states.dim() == 2 and root_states.shape[1] == 13 and root_states.stride(1) == 1, \
            "proj_launch: root_states f32 [n, 13], unit column stride"
        n = root_states.shape[0]
        for who, t in (('body_pos', body_pos), ('body_vel', body_vel)):
            assert t.dtype == f32 and t.dim() == 3 and t.shape[0] == n and t.shape[2] == 3 and t.stride(2) == 1, \
                f"proj_launch: {who} f32 [n, B, 3], unit stride in the last dimension"
        assert body_vel.shape == body_pos.shape, "proj_launch: body_vel shaped like body_pos"
        assert proj_states.dtype == f32 and proj_states.dim() == 3 and proj_states.shape[0] == n and proj_states.shape[2] == 13 and \
            proj_states.stride(2) == 1, "proj_launch: proj_states f32 [n, K, 13], unit stride in the last dimension"
        K = proj_states.shape[1]
        n_slots = K
        if timesteps is not None:
            assert timesteps.dtype == torch.int32 and timesteps.dim() == 1 and timesteps.is_contiguous() and 1 <= timesteps.numel() <= K, \
                "proj_launch: timesteps int32 [n_slots], n_slots at most the projectiles of proj_states"
            n_slots = timesteps.numel()
        assert progress_buf is None or (progress_buf.dtype == torch.int64 and progress_buf.is_contiguous() and progress_buf.numel() == n), \
            "proj_launch: progress_buf int64 [n]"
        assert int(slot) < n_slots, f"proj_launch: slot {slot} beyond the {n_slots} projectiles"
        n_ids = 0
        if env_ids is not None:
            assert env_ids.dtype == torch.int32 and env_ids.is_contiguous() and env_ids.dim() == 1, "proj_launch: env_ids contiguous int32"
            n_ids = env_ids.numel()
            if n_ids == 0 and (rng_state is None or not advance) and slot_out is None:
                return
        rows = n_ids if env_ids is not None else n
        assert u is None or (u.dtype == f32 and u.shape == (rows, 4) and u.is_contiguous()), "proj_launch: u f32 [rows, 4]"
        assert eps is None or (eps.dtype == f32 and eps.shape == (rows, 3) and eps.is_contiguous()), "proj_launch: eps f32 [rows, 3]"
        assert rng_state is None or (rng_state.dtype == torch.int64 and rng_state.numel() == 2 and rng_state.is_contiguous()), \
            "proj_launch: rng_state int64 [2]"
        assert slot_out is None or (slot_out.dtype == torch.int32 and slot_out.numel() == 1), "proj_launch: slot_out int32 [1]"
        assert ids_out is None or (ids_out.dtype == torch.int32 and ids_out.numel() == n and ids_out.is_contiguous()), \
            "proj_launch: ids_out int32 [n]"
        assert draws_out is None or (draws_out.dtype == f32 and draws_out.shape == (n, L.PROJ_DRAWS) and draws_out.is_contiguous()), \
            "proj_launch: draws_out f32 [n, 7]"
        # an empty tensor has no storage: an empty id list is still ids mode, so it gets a pointer (that is never read)
        ids_ptr = _ptr(root_states) if env_ids is not None and n_ids == 0 else _ptr(env_ids)
        L.check(self.lib.ase_hip_proj_launch(_ptr(progress_buf), _ptr(timesteps), n_slots, int(slot), ids_ptr, n_ids, _ptr(u), _ptr(eps),
                                             _ptr(rng_state), int(advance), _ptr(root_states), root_states.stride(0), _ptr(body_pos),
                                             body_pos.stride(0), body_pos.stride(1), _ptr(body_vel), body_vel.stride(0),
                                             body_vel.stride(1), body_pos.shape[1], int(tar_body), _ptr(proj_states),
                                             proj_states.stride(0), proj_states.stride(1), float(dist_min), float(dist_max),
                                             float(h_min), float(h_max), float(speed_min), float(speed_max), float(noise),
                                             _ptr(slot_out), _ptr(ids_out), _ptr(draws_out), n, self._stream()), "proj_launch")

    # ------------------------------------------------------------------ the view-motion task (N17)
    def motion_sync(self, clips, motion_ids, progress_buf, reset_buf, terminate_buf, mode=L.MOTION_SYNC, motion_dt=0.0,
                    root_states=None, dof_pos=None, dof_vel=None, body_pos=None, body_rot=None, body_vel=None, body_ang_vel=None,
                    env_ids=None, ids_out=None):
        """HumanoidViewMotion's per-step logic in one launch (operands: see ase_hip_motion_sync).  clips: the dict of
        ``motion_state``; motion_ids int32 [n], progress_buf / reset_buf / terminate_buf int64 [n], all written in place.
        mode L.MOTION_SYNC: reset_buf = progress_buf * motion_dt > clip length (strict), terminate_buf = 0, and the pose of
        (motion_ids, progress_buf * motion_dt) written in place - root_states f32 [n, 13] at any row stride (its velocities
        zeroed), dof_pos / dof_vel f32 [n, D] at any environment and element stride (dof_vel zeroed), and the optional
        body_pos / body_vel / body_ang_vel [n, B, 3] and body_rot [n, B, 4] at their own strides: the clip's global arrays
        blended by the sampler's two expressions, velocities zero.  mode L.MOTION_RESET: for the rows with reset_buf != 0, or
        for env_ids (int32, distinct, -1: skip), motion_ids = (motion_ids + n) % num_motions and the three buffers cleared; no
        state operand; ids_out int32 [n] (not with env_ids) receives e for a reset row and -1 elsewhere.  The entry takes raw
        addresses: every tensor lives on the backend's device.  Recordable in a launch program."""
        f32, i64, i32 = torch.float32, torch.int64, torch.int32
        n = motion_ids.numel()
        B, D, J = clips['gts'].shape[1], int(clips['dof_offsets'][-1]), len(clips['dof_body_ids'])
        tensors = dict(motion_ids=motion_ids, progress_buf=progress_buf, reset_buf=reset_buf, terminate_buf=terminate_buf,
                       root_states=root_states, dof_pos=dof_pos, dof_vel=dof_vel, body_pos=body_pos, body_rot=body_rot, body_vel=body_vel,
                       body_ang_vel=body_ang_vel, env_ids=env_ids, ids_out=ids_out)
        for who, t in tensors.items():
            assert t is None or self._here(t), f"motion_sync: {who} must be a tensor on {self.device}, not {t.device}"
        assert motion_ids.dtype == i32 and motion_ids.is_contiguous() and motion_ids.dim() == 1, "motion_sync: motion_ids contiguous int32 [n]"
        bufs = [self._dense(t, n, i64, who) for t, who in ((progress_buf, 'progress_buf'), (reset_buf, 'reset_buf'),
                                                           (terminate_buf, 'terminate_buf'))]
        ids_out_p = self._dense(ids_out, n, i32, 'ids_out')
        ids_p, n_ids = None, 0
        if env_ids is not None:
            assert env_ids.dtype == i32 and env_ids.is_contiguous() and env_ids.dim() == 1, "motion_sync: env_ids contiguous int32"
            n_ids = env_ids.numel()
            if n_ids == 0:                                    # an empty tensor has no storage: an empty list resets nothing
                return
            ids_p = _ptr(env_ids)
        rs, rs_stride = self._state_rows(root_states, n, 13, 'root_states')
        dofs = []
        for t, who in ((dof_pos, 'dof_pos'), (dof_vel, 'dof_vel')):
            assert t is None or (t.dtype == f32 and tuple(t.shape) == (n, D)), f"motion_sync: {who} f32 [{n}, {D}]"
            dofs += [None, 0, 0] if t is None else [_ptr(t), int(t.stride(0)), int(t.stride(1))]
        bodies = []
        for t, w, who in ((body_pos, 3, 'body_pos'), (body_rot, 4, 'body_rot'), (body_vel, 3, 'body_vel'), (body_ang_vel, 3, 'body_ang_vel')):
            bodies += [None, 0, 0] if t is None else list(self._state_view(t, (n, B, w), who))
        ia = lambda xs: self._id_array(xs)[0]
        L.check(self.lib.ase_hip_motion_sync(int(mode), _ptr(clips['gts']), _ptr(clips['grs']), _ptr(clips['lrs']), B, _ptr(clips['lengths']),
                                             _ptr(clips['num_frames']), _ptr(clips['dt']), _ptr(clips['length_starts']),
                                             clips['lengths'].numel(), ia(clips['dof_body_ids']), ia(clips['dof_offsets']), J,
                                             _ptr(motion_ids), bufs[0], float(motion_dt), bufs[1], bufs[2], rs, rs_stride, *dofs, *bodies,
                                             ids_p, n_ids, ids_out_p, n, self._stream()), "motion_sync")

    # ------------------------------------------------------------------ renewals of the ASE latents (N9)
    def latent_renew(self, latents, env_ids=None, eps=None, steps=None, rng_state=None, advance=True, progress_buf=None,
                     reset_steps=None, steps_add=False, steps_low=0, steps_high=1, z2=None):
        """_reset_latents / _reset_latent_step_count / _update_latents in one launch (operands: see ase_hip_latent_renew).
        env_ids (int32, distinct) names the rows, None: every environment with reset_steps <= progress_buf (int32 or int64).
        The draws are either passed in (eps f32 [n_ids, >= dim], steps int32 [n_ids] when reset_steps is given) or made on
        the device from rng_state (int64 [2] = seed | offset, advanced by one unless advance is false).  latents
        [n_envs, dim] f32 and reset_steps int32 [n_envs] are written in place; z2 (due mode: every environment's latent after
        the decision, f32 / f16 / bf16) too.  latents, eps and z2 may be strided views with unit column stride."""
        assert latents.dtype == torch.float32 and latents.dim() == 2 and latents.stride(1) == 1, "latents: f32 [n_envs, dim], unit column stride"
        n, dim = latents.shape
        n_ids = 0
        if env_ids is not None:
            assert env_ids.dtype == torch.int32 and env_ids.is_contiguous() and env_ids.dim() == 1, "env_ids: contiguous int32 vector"
            n_ids = env_ids.numel()
            if n_ids == 0 and (rng_state is None or not advance):
                return                                   # nothing to renew and no stream position to move
        assert eps is None or (eps.dtype == torch.float32 and eps.dim() == 2 and eps.shape[0] == n_ids and eps.shape[1] >= dim and
                               eps.stride(1) == 1), "eps: f32 [n_ids, >= dim], unit column stride"
        assert steps is None or (steps.dtype == torch.int32 and steps.is_contiguous() and steps.shape == (n_ids,)), "steps: int32 [n_ids]"
        assert reset_steps is None or (reset_steps.dtype == torch.int32 and reset_steps.is_contiguous() and
                                       reset_steps.shape == (n,)), "reset_steps: int32 [n_envs]"
        assert progress_buf is None or (progress_buf.dtype in (torch.int32, torch.int64) and progress_buf.is_contiguous() and
                                        progress_buf.shape == (n,)), "progress_buf: int32 or int64 [n_envs]"
        assert rng_state is None or (rng_state.dtype == torch.int64 and rng_state.numel() == 2 and rng_state.is_contiguous())
        assert z2 is None or (z2.dim() == 2 and z2.shape == (n, dim) and z2.stride(1) == 1), "z2: [n_envs, dim], unit column stride"
        # an empty tensor has no storage: an empty id list is still ids mode, so it gets a pointer (that is never read)
        ids_ptr = _ptr(latents) if env_ids is not None and n_ids == 0 else _ptr(env_ids)
        L.check(self.lib.ase_hip_latent_renew(ids_ptr, n_ids, _ptr(eps), _ld(eps), _ptr(steps), _ptr(rng_state), int(advance),
                                              _ptr(progress_buf), int(progress_buf is not None and progress_buf.dtype == torch.int64),
                                              _ptr(reset_steps), int(bool(steps_add)), int(steps_low), int(steps_high),
                                              _ptr(latents), _ld(latents), _ptr(z2), _ld(z2), 0 if z2 is None else _code(z2.dtype),
                                              n, dim, self._stream()), "latent_renew")

    # ------------------------------------------------------------------ resets (N6)
    def amp_reset(self, clips, env_ids, kind, motion_ids, motion_times, src_rows, table, root_states, dof_pos, dof_vel, body_pos,
                  body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs, env_dt, hist,
                  kinds=L.RESET_HAS_TABLE | L.RESET_HAS_MOTION):
        """HumanoidAMP / HumanoidAMPGetup resets in one launch (env/tasks/humanoid_amp.py:141-246, humanoid_amp_getup.py:
        109-129; operands: see ase_hip_amp_reset).  clips: the dict of motion_state (its python lists dof_offsets /
        key_body_ids are always read, dof_body_ids and the tensors only with RESET_HAS_MOTION in kinds).  The plan arrays
        env_ids / kind / motion_ids / src_rows (int32) and motion_times (f32) have one element per reset row; table =
        (root_states [T, 13], dof_pos [T, D], dof_vel [T, D]) or None.  root_states [N, 13], dof_pos / dof_vel [N, D] are
        written in place and may be strided views (dof: both with the same strides, element stride 1 or 2); hist [N, S, F]."""
        n, S, F = hist.shape
        B, D = body_pos.shape[1], int(clips['dof_offsets'][-1])
        J, K = len(clips['dof_offsets']) - 1, len(clips['key_body_ids'])
        has_table, has_motion = bool(kinds & L.RESET_HAS_TABLE), bool(kinds & L.RESET_HAS_MOTION)
        ia = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])
        self._f32c(body_pos, body_rot, body_vel, body_ang_vel, hist)
        assert body_rot.shape == (n, B, 4) and body_vel.shape == body_ang_vel.shape == body_pos.shape == (n, B, 3)
        assert F == 13 + 6 * J + D + 3 * K, "hist: [n_envs, n_steps, 13 + 6 J + D + 3 K]"
        n_ids = env_ids.numel()
        for t, dt in ((env_ids, torch.int32), (kind, torch.int32), (motion_ids, torch.int32), (src_rows, torch.int32),
                      (motion_times, torch.float32)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and t.numel() == n_ids), "plan: int32 / f32 [n_ids]"
        for t in (root_states, dof_pos, dof_vel):
            assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == n
        assert root_states.shape[1] == 13 and root_states.stride(1) == 1
        assert dof_pos.shape == dof_vel.shape == (n, D) and dof_pos.stride() == dof_vel.stride()
        tab = (None, None, None)
        if has_table:
            tab = table
            self._f32c(*tab)
            assert tab[0].dim() == 2 and tab[0].shape[1] == 13 and tab[1].shape == tab[2].shape == (tab[0].shape[0], D)
        cl = {k: (clips[k] if has_motion else None) for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'num_frames',
                                                                'dt', 'length_starts')}
        assert not has_motion or cl['gts'].shape[1] == B, "the clips' skeleton is the simulator's"
        L.check(self.lib.ase_hip_amp_reset(_ptr(cl['gts']), _ptr(cl['grs']), _ptr(cl['lrs']), _ptr(cl['grvs']), _ptr(cl['gravs']),
                                           _ptr(cl['dvs']), B, _ptr(cl['lengths']), _ptr(cl['num_frames']), _ptr(cl['dt']),
                                           _ptr(cl['length_starts']), ia(clips['dof_body_ids']) if has_motion else None,
                                           ia(clips['dof_offsets']), J, ia(clips['key_body_ids']), K, _ptr(env_ids), _ptr(kind),
                                           _ptr(motion_ids), _ptr(motion_times), _ptr(src_rows), n_ids, int(kinds), _ptr(tab[0]),
                                           _ptr(tab[1]), _ptr(tab[2]), 0 if tab[0] is None else tab[0].shape[0],
                                           _ptr(root_states), root_states.stride(0), _ptr(dof_pos), _ptr(dof_vel), dof_pos.stride(0),
                                           dof_pos.stride(1), _ptr(body_pos), _ptr(body_rot), _ptr(body_vel), _ptr(body_ang_vel), n,
                                           int(local_root_obs), int(root_height_obs), float(env_dt), _ptr(hist), S, self._stream()),
                "amp_reset")

    def amp_reset_due(self, clips, clip_cdf, table, state_init, hybrid_init_prob, getup, rng_state, progress_buf, reset_buf,
                      terminate_buf, recovery_counter, plan, root_states, dof_pos, dof_vel, body_pos, body_rot, body_vel,
                      body_ang_vel, local_root_obs, root_height_obs, env_dt, hist, advance=True):
        """The resets of amp_reset with the due test and the draws inside the launch (N10; operands and the draw table: see
        ase_hip_amp_reset_due): every environment with reset_buf != 0 is reset, its draws depend on (seed, stream position,
        environment) only.  state_init: L.INIT_*; getup: None or (recovery_episode_prob, recovery_steps, fall_init_prob),
        then terminate_buf and recovery_counter (int32 [N]) are needed.  clips / table as for amp_reset (the clip tensors
        and clip_cdf, uint32 bits in an int32 [n_clips] tensor, unless state_init is INIT_DEFAULT; the table for INIT_DEFAULT /
        INIT_HYBRID and fall episodes, fall states behind the N initial rows).  rng_state int64 [2] = seed | offset, advanced
        by one unless advance is false.  progress_buf / reset_buf / terminate_buf (int64 [N]; progress_buf and, without
        getup, terminate_buf may be None), recovery_counter and the state are written in place, for the reset rows only.
        plan: None or the dict of five [N] tensors (env_ids, kind, motion_ids, src_rows int32, motion_times f32) that receives
        every environment's decision, env_ids -1 where none was made."""
        n, S, F = hist.shape
        B, D = body_pos.shape[1], int(clips['dof_offsets'][-1])
        J, K = len(clips['dof_offsets']) - 1, len(clips['key_body_ids'])
        has_motion = state_init != L.INIT_DEFAULT
        ia = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])
        self._f32c(body_pos, body_rot, body_vel, body_ang_vel, hist)
        assert body_rot.shape == (n, B, 4) and body_vel.shape == body_ang_vel.shape == body_pos.shape == (n, B, 3)
        assert F == 13 + 6 * J + D + 3 * K, "hist: [n_envs, n_steps, 13 + 6 J + D + 3 K]"
        for t in (progress_buf, reset_buf, terminate_buf):
            assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.shape == (n,)), "buffers: int64 [n_envs]"
        assert recovery_counter is None or (recovery_counter.dtype == torch.int32 and recovery_counter.is_contiguous() and
                                            recovery_counter.shape == (n,)), "recovery_counter: int32 [n_envs]"
        assert rng_state is None or (rng_state.dtype == torch.int64 and rng_state.numel() == 2 and rng_state.is_contiguous())
        out = {k: None for k in ('env_ids', 'kind', 'motion_ids', 'motion_times', 'src_rows')} if plan is None else plan
        for k, t in out.items():
            assert t is None or (t.dtype == (torch.float32 if k == 'motion_times' else torch.int32) and t.is_contiguous() and
                                 t.shape == (n,)), "plan: int32 / f32 [n_envs]"
        for t in (root_states, dof_pos, dof_vel):
            assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == n
        assert root_states.shape[1] == 13 and root_states.stride(1) == 1
        assert dof_pos.shape == dof_vel.shape == (n, D) and dof_pos.stride() == dof_vel.stride()
        tab = (None, None, None)
        if table is not None:
            tab = table
            self._f32c(*tab)
            assert tab[0].dim() == 2 and tab[0].shape[1] == 13 and tab[1].shape == tab[2].shape == (tab[0].shape[0], D)
        cl = {k: (clips[k] if has_motion else None) for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'num_frames',
                                                                'dt', 'length_starts')}
        n_clips = 0
        if has_motion:
            assert cl['gts'].shape[1] == B, "the clips' skeleton is the simulator's"
            n_clips = cl['lengths'].numel()
            assert clip_cdf is not None and clip_cdf.dtype == torch.int32 and clip_cdf.is_contiguous() and \
                clip_cdf.shape == (n_clips,), "clip_cdf: int32 [n_clips]"
        rec_prob, rec_steps, fall_prob = (0.0, 0, 0.0) if getup is None else getup
        L.check(self.lib.ase_hip_amp_reset_due(_ptr(cl['gts']), _ptr(cl['grs']), _ptr(cl['lrs']), _ptr(cl['grvs']), _ptr(cl['gravs']),
                                               _ptr(cl['dvs']), B, _ptr(cl['lengths']), _ptr(cl['num_frames']), _ptr(cl['dt']),
                                               _ptr(cl['length_starts']), ia(clips['dof_body_ids']) if has_motion else None,
                                               ia(clips['dof_offsets']), J, ia(clips['key_body_ids']), K,
                                               _ptr(clip_cdf) if has_motion else None, n_clips, _ptr(tab[0]), _ptr(tab[1]),
                                               _ptr(tab[2]), 0 if tab[0] is None else tab[0].shape[0], int(state_init),
                                               float(hybrid_init_prob), int(getup is not None), float(rec_prob), float(fall_prob),
                                               int(rec_steps), _ptr(rng_state), int(advance), _ptr(progress_buf), _ptr(reset_buf),
                                               _ptr(terminate_buf), _ptr(recovery_counter), _ptr(out['env_ids']), _ptr(out['kind']),
                                               _ptr(out['motion_ids']), _ptr(out['motion_times']), _ptr(out['src_rows']),
                                               _ptr(root_states), root_states.stride(0), _ptr(dof_pos), _ptr(dof_vel),
                                               dof_pos.stride(0), dof_pos.stride(1), _ptr(body_pos), _ptr(body_rot), _ptr(body_vel),
                                               _ptr(body_ang_vel), n, int(local_root_obs), int(root_height_obs), float(env_dt),
                                               _ptr(hist), S, self._stream()), "amp_reset_due")

    # ------------------------------------------------------------------ demo fetch (N11)
    def amp_demo_fetch(self, clips, out, ring_rows, head, n, num_steps, truncate_time, dt, local_root_obs, root_height_obs,
                       motion_ids=None, motion_times0=None, rng_state=None, clip_cdf=None, advance=True, draws_out=None,
                       head_dev=None):
        """HumanoidAMP.fetch_amp_obs_demo + build_amp_obs_demo and the store into the demo ring in one launch (env/tasks/
        humanoid_amp.py:63-105; operands and the draw table: see ase_hip_amp_demo_fetch).  clips: the dict of motion_state.
        out: f32 [ring_rows, >= num_steps * F] with unit column stride (any row stride); sample i goes to row (head + i) %
        ring_rows.  Either motion_ids (int32 [n]) and motion_times0 (f32 [n]) are passed in, or rng_state (int64 [2] = seed |
        offset, advanced by one unless advance is false) and clip_cdf (uint32 bits in an int32 [n_clips] tensor) draw them on
        the device.  draws_out: None or (int32 [n], f32 [n]) receiving every sample's clip and time.  head_dev: None or an int32
        [1] device tensor added to head when the launch runs."""
        B, D = clips['gts'].shape[1], int(clips['dof_offsets'][-1])
        J, K = len(clips['dof_offsets']) - 1, len(clips['key_body_ids'])
        n, S, F = int(n), int(num_steps), 13 + 6 * J + D + 3 * K
        n_clips = clips['lengths'].numel()
        ia = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])
        assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1, "out: f32 [ring_rows, >= n_steps * F] rows"
        assert out.shape[0] >= ring_rows and out.shape[1] >= S * F and out.stride(0) >= S * F, "out: ring_rows rows of n_steps * F columns"
        for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'dt'):
            assert clips[k].dtype == torch.float32 and clips[k].is_contiguous()
        for k in ('num_frames', 'length_starts'):
            assert clips[k].dtype == torch.int32 and clips[k].is_contiguous() and clips[k].numel() == n_clips
        assert clips['dt'].numel() == n_clips and len(clips['dof_body_ids']) == J
        for t, dtype in ((motion_ids, torch.int32), (motion_times0, torch.float32)):
            assert t is None or (t.dtype == dtype and t.is_contiguous() and t.shape == (n,)), "draws: int32 / f32 [n]"
        assert rng_state is None or (rng_state.dtype == torch.int64 and rng_state.numel() == 2 and rng_state.is_contiguous())
        assert clip_cdf is None or (clip_cdf.dtype == torch.int32 and clip_cdf.is_contiguous() and clip_cdf.shape == (n_clips,)), \
            "clip_cdf: int32 [n_clips]"
        ids_out, times_out = (None, None) if draws_out is None else draws_out
        for t, dtype in ((ids_out, torch.int32), (times_out, torch.float32)):
            assert t is None or (t.dtype == dtype and t.is_contiguous() and t.shape == (n,)), "draws_out: int32 / f32 [n]"
        assert head_dev is None or (head_dev.dtype == torch.int32 and head_dev.numel() == 1)
        L.check(self.lib.ase_hip_amp_demo_fetch(_ptr(clips['gts']), _ptr(clips['grs']), _ptr(clips['lrs']), _ptr(clips['grvs']),
                                                _ptr(clips['gravs']), _ptr(clips['dvs']), B, _ptr(clips['lengths']),
                                                _ptr(clips['num_frames']), _ptr(clips['dt']), _ptr(clips['length_starts']), n_clips,
                                                ia(clips['dof_body_ids']), ia(clips['dof_offsets']), J, ia(clips['key_body_ids']), K,
                                                _ptr(motion_ids), _ptr(motion_times0), _ptr(rng_state), _ptr(clip_cdf), int(advance),
                                                _ptr(ids_out), _ptr(times_out), n, S, float(truncate_time), float(dt),
                                                int(local_root_obs), int(root_height_obs), _ptr(out), out.stride(0), int(ring_rows),
                                                int(head), _ptr(head_dev), self._stream()), "amp_demo_fetch")

    # ------------------------------------------------------------------ one environment step into the experience (N12)
    _KINDS = {torch.uint8: L.KIND_U8, torch.bool: L.KIND_U8, torch.int32: L.KIND_I32, torch.int64: L.KIND_I64,
              torch.float32: L.KIND_F32}

    def _rollout_store_table(self, n, n_slots, fields):
        """The device field table of rollout_store, kept per field set (addresses and pitches; the slot is no part of it).
        A new set is uploaded from pinned memory without waiting for the copy.  A table is never dropped: a launch program that
        recorded a call holds its address (768 bytes at most per set).  Only addresses on this backend's device enter it."""
        rows = []
        for src, dst in fields:
            assert self._here(src) and self._here(dst), \
                f"fields: tensors on {self.device} (the table holds raw addresses the kernel dereferences)"
            assert src.dtype == torch.float32 and dst.dtype == torch.float32, "fields: f32"
            src = src.view(n, -1) if src.dim() != 2 else src
            D = src.shape[1]
            assert src.shape[0] == n and D >= 1 and (D == 1 or src.stride(1) == 1) and src.stride(0) >= D, "field source: [n_envs, D] rows"
            dst = dst.view(dst.shape[0], n, -1) if dst.dim() != 3 else dst
            assert dst.shape == (n_slots, n, D) and (D == 1 or dst.stride(2) == 1) and dst.stride(1) >= D and \
                dst.stride(0) >= n * dst.stride(1), "field destination: [n_slots, n_envs, D] rows"
            rows.append((src.data_ptr(), src.stride(0), D, dst.data_ptr(), dst.stride(1), dst.stride(0)))
        key = tuple(rows)
        tabs = self.__dict__.setdefault('_rs_tables', {})
        hit = tabs.get(key)
        if hit is None:
            hit = tabs[key] = torch.tensor(rows, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
        return hit

    def rollout_store(self, dones, slot=0, n_slots=None, fields=(), rewards=None, shift=0.0, scale=1.0, rewards_out=None,
                      dones_out=None, next_values=None, terminate=None, next_values_out=None, cur_rewards=None,
                      cur_lengths=None, meter=None, max_size=0, workspace=None, done_ids_out=None, slot_dev=None):
        """What play_steps does behind env_step, for experience slot `slot`, in one entry (learning/common_agent.py:267-293;
        operands: see ase_hip_rollout_store).  dones [n_envs] uint8 / bool / int32 / int64 / f32.  fields: (source [n_envs, D],
        destination [n_slots, n_envs, D]) pairs of f32 tensors with unit column stride, at most 16.  rewards f32 [n_envs];
        rewards_out / next_values_out f32 and dones_out uint8 are [n_slots, n_envs(, 1)] buffers, next_values f32 [n_envs] with
        terminate typed like dones.  cur_rewards / cur_lengths f32 [n_envs] are updated in place and come with meter (f64 [4] =
        reward mean, length mean, current size, episodes seen) and max_size; workspace (f64, lib.rollout_store_ws(n_envs)) is
        the backend's own when None, one per size and stream.  Every tensor lives on the backend's device.  done_ids_out int32 [n_envs].  slot_dev: None or an int32 [1] device tensor read when the
        launch runs, in place of slot.  Recordable in a launch program."""
        n = dones.numel()
        vec = lambda t, dt, who: None if t is None else self._rs_vec(t, n, dt, who)
        dones, terminate = vec(dones, None, 'dones'), vec(terminate, None, 'terminate')
        rewards, next_values = vec(rewards, torch.float32, 'rewards'), vec(next_values, torch.float32, 'next_values')
        cur_rewards, cur_lengths = vec(cur_rewards, torch.float32, 'cur_rewards'), vec(cur_lengths, torch.float32, 'cur_lengths')
        done_ids_out = vec(done_ids_out, torch.int32, 'done_ids_out')
        slotted = [(rewards_out, torch.float32), (dones_out, torch.uint8), (next_values_out, torch.float32)]
        for t, dt in slotted:
            if t is not None:
                assert self._here(t), f"slotted output: a tensor on {self.device}"
                assert t.dtype == dt and t.dim() >= 2 and t[0].numel() == n and t.shape[1] == n and t.stride(1) == 1, \
                    "slotted output: [n_slots, n_envs(, 1)], unit stride over the environments"
                assert n_slots is None or n_slots == t.shape[0], "outputs disagree on n_slots"
                n_slots = t.shape[0]
        if n_slots is None:
            n_slots = fields[0][1].shape[0] if fields else 1
        table = self._rollout_store_table(n, n_slots, fields) if fields else None
        assert meter is None or (meter.dtype == torch.float64 and meter.numel() == 4 and meter.is_contiguous() and
                                 self._here(meter)), "meter: f64 [4] on the device"
        if meter is not None and workspace is None:
            # private to a call until it completes: calls of one stream are ordered, so the backend keeps one per stream
            ws, key = self.__dict__.setdefault('_rs_ws', {}), (n, torch.cuda.current_stream(self.device).cuda_stream)
            workspace = ws.get(key)
            if workspace is None:
                workspace = ws[key] = torch.zeros(L.rollout_store_ws(n), dtype=torch.float64, device=self.device)
        assert workspace is None or (workspace.dtype == torch.float64 and workspace.is_contiguous() and
                                     self._here(workspace)), "workspace: f64 on the device"
        assert slot_dev is None or (slot_dev.dtype == torch.int32 and slot_dev.numel() == 1 and self._here(slot_dev))
        kind = lambda t: 0 if t is None else self._KINDS[t.dtype]
        L.check(self.lib.ase_hip_rollout_store(_ptr(table), len(fields), _ptr(rewards), float(shift), float(scale),
                                               _ptr(rewards_out), _ld(rewards_out), _ptr(dones), kind(dones), _ptr(dones_out),
                                               _ld(dones_out), _ptr(next_values), _ptr(terminate), kind(terminate),
                                               _ptr(next_values_out), _ld(next_values_out), _ptr(cur_rewards), _ptr(cur_lengths),
                                               _ptr(meter), int(max_size), _ptr(workspace),
                                               0 if workspace is None else workspace.numel(), _ptr(done_ids_out), n, int(slot),
                                               _ptr(slot_dev), int(n_slots), self._stream()), "rollout_store")

    # ------------------------------------------------------------------ the head of a rollout step (N18)
    def rollout_head(self, obs, z=None, mean=None, std=None, xa=None, xc=None, zc=None, zs=None, obses_out=None, z_out=None,
                     slot=0, slot_dev=None):
        """The head of one environment step in one launch (operands: see ase_hip_rollout_head).  obs f32 [n, D] and z f32
        [n, Z] (optional) are read at their own pitch.  xa / xc [n, >= D] receive the eval-mode normalisation of obs with
        mean / std f32 [D] (columns beyond D untouched), zc / zs [n, >= Z] the latents converted as gather_rows converts them;
        the four share one dtype (f32 / bf16 / f16).  obses_out f32 [n_slots, n, D] and z_out f32 [n_slots, n, Z] receive the
        raw rows of slot `slot`, or of the int32 [1] device word slot_dev read when the launch runs (a word outside the
        buffer: the whole call writes nothing).  Every output is optional, one is required; every tensor has unit column
        stride and lives on the backend's device (the entry takes raw addresses).  Recordable in a launch program."""
        f32 = torch.float32
        for who, t in dict(obs=obs, z=z, mean=mean, std=std, xa=xa, xc=xc, zc=zc, zs=zs, obses_out=obses_out, z_out=z_out,
                           slot_dev=slot_dev).items():
            assert t is None or self._here(t), f"rollout_head: {who} must be a tensor on {self.device}, not {t.device}"
        assert obs.dim() == 2 and obs.dtype == f32 and obs.stride(1) == 1, "rollout_head: obs f32 [n, D], unit column stride"
        n, D = obs.shape
        Z = 0
        if z is not None:
            assert z.dim() == 2 and z.dtype == f32 and z.shape[0] == n and z.stride(1) == 1, "rollout_head: z f32 [n, Z], unit column stride"
            Z = z.shape[1]
        for who, t in (('mean', mean), ('std', std)):
            assert t is None or (t.dtype == f32 and t.numel() == D and t.is_contiguous()), f"rollout_head: {who} contiguous f32 [D]"
        xs = [t for t in (xa, xc, zc, zs) if t is not None]
        assert all(t.dtype == xs[0].dtype for t in xs), "rollout_head: xa / xc / zc / zs share one dtype"
        for who, t, w in (('xa', xa, D), ('xc', xc, D), ('zc', zc, Z), ('zs', zs, Z)):
            assert t is None or (t.dim() == 2 and t.shape[0] == n and t.shape[1] >= w and t.stride(1) == 1), \
                f"rollout_head: {who} [n, >= {w}], unit column stride"
        n_slots = 1
        for who, t, w in (('obses_out', obses_out, D), ('z_out', z_out, Z)):
            if t is not None:
                assert t.dtype == f32 and t.dim() == 3 and tuple(t.shape[1:]) == (n, w) and t.stride(2) == 1, \
                    f"rollout_head: {who} f32 [n_slots, n, {w}], unit column stride"
                n_slots = t.shape[0]
        assert obses_out is None or z_out is None or obses_out.shape[0] == z_out.shape[0], "rollout_head: outputs disagree on n_slots"
        assert slot_dev is None or (slot_dev.dtype == torch.int32 and slot_dev.numel() == 1), "rollout_head: slot_dev int32 [1]"
        # (the row stride of a one-row view means nothing - 0 or 1 after a select or an expand: its width stands in for it)
        ld = lambda t: 0 if t is None else (max(int(t.stride(0)), int(t.shape[1])) if n == 1 else int(t.stride(0)))
        sl = lambda t: (None, 0, 0) if t is None else (_ptr(t), max(int(t.stride(1)), int(t.shape[2])) if n == 1 else int(t.stride(1)),
                                                       int(t.stride(0)))
        L.check(self.lib.ase_hip_rollout_head(_ptr(obs), ld(obs), D, _ptr(z), ld(z), Z, _ptr(mean), _ptr(std), _ptr(xa), ld(xa),
                                              _ptr(xc), ld(xc), _ptr(zc), ld(zc), _ptr(zs), ld(zs),
                                              _code(xs[0].dtype) if xs else L.F32, *sl(obses_out), *sl(z_out), n, int(slot),
                                              _ptr(slot_dev), n_slots, self._stream()), "rollout_head")

    def word_step(self, word, add=1, wrap=0):
        """word[0] = (word[0] + add) mod wrap on the device, one lane (wrap <= 0: no modulo): the step counter of a recorded
        rollout step, the word rollout_store and rollout_head read their slot from.  word: int32 [1] on the backend's device."""
        assert self._here(word) and word.dtype == torch.int32 and word.numel() == 1, f"word_step: word int32 [1] on {self.device}"
        L.check(self.lib.ase_hip_word_step(_ptr(word), int(add), int(wrap), self._stream()), "word_step")

    def _here(self, t):
        """Whether a tensor lives on this backend's GPU (a device given without an index is the current one)."""
        return t.is_cuda and t.device.index == (torch.cuda.current_device() if self.device.index is None else self.device.index)

    def _rs_vec(self, t, n, dtype, who):
        cls = type(self)
        assert self._here(t), f"{who}: a tensor on {self.device}, not {t.device}"
        assert t.numel() == n and t.is_contiguous() and (t.dtype == dtype if dtype is not None else t.dtype in cls._KINDS), \
            f"{who}: contiguous [n_envs] of {dtype or 'uint8 / bool / int32 / int64 / float32'}"
        return t

    # ------------------------------------------------------------------ the HRL inner loop's glue (N13)
    def _hrl_rows(self, t, n, cols, dtype, who):
        """[n, >= cols] rows of `dtype` with unit column stride on this GPU: the kernels dereference raw addresses at t's pitch."""
        assert self._here(t), f"{who}: a tensor on {self.device}, not {t.device}"
        assert t.dim() == 2 and t.shape[0] == n and t.shape[1] >= cols and t.stride(1) == 1 and t.stride(0) >= cols and \
            (t.dtype == dtype if dtype is not None else t.dtype in (torch.float32, torch.bfloat16, torch.float16)), \
            f"{who}: [{n}, >= {cols}] rows of {dtype or 'f32 / bf16 / f16'}, unit column stride"
        return t

    def hrl_latent(self, actions, z=None, z2=None, dim=None):
        """z = normalize(clamp(actions, -1, 1)) per row (ase_hip_hrl_latent): actions f32 [n, >= dim]; z f32 [n, >= dim] and / or
        z2 [n, >= dim] in f32 / bf16 / f16 (the style chain's input buffer: columns [0, dim) only), each read or written at its
        own pitch.  dim defaults to actions' width.  Recordable in a launch program."""
        n = actions.shape[0]
        dim = actions.shape[1] if dim is None else int(dim)
        f32 = torch.float32
        actions = self._hrl_rows(actions, n, dim, f32, 'actions')
        z = None if z is None else self._hrl_rows(z, n, dim, f32, 'z')
        z2 = None if z2 is None else self._hrl_rows(z2, n, dim, None, 'z2')
        assert z is not None or z2 is not None, "hrl_latent: z or z2"
        L.check(self.lib.ase_hip_hrl_latent(_ptr(actions), _ld(actions), _ptr(z), _ld(z), _ptr(z2), _ld(z2),
                                            0 if z2 is None else _code(z2.dtype), n, dim, self._stream()), "hrl_latent")

    def hrl_llc_action(self, mu, low, high, out, act, clip=True):
        """The padded head output mu f32 [n, >= act] -> out f32 [n, >= act]: clamp(mu, -1, 1) * ((high - low) / 2) +
        ((high + low) / 2) with clip, a strided copy without (ase_hip_hrl_llc_action).  low / high f32 [act], contiguous."""
        n, act, f32 = mu.shape[0], int(act), torch.float32
        mu, out = self._hrl_rows(mu, n, act, f32, 'mu'), self._hrl_rows(out, n, act, f32, 'out')
        for t, who in ((low, 'low'), (high, 'high')):
            assert (t is None and not clip) or (self._here(t) and t.dtype == f32 and t.numel() == act and t.is_contiguous()), \
                f"{who}: contiguous f32 [{act}] on {self.device}"
        L.check(self.lib.ase_hip_hrl_llc_action(_ptr(mu), _ld(mu), _ptr(low), _ptr(high), _ptr(out), _ld(out), n, act, int(bool(clip)),
                                                self._stream()), "hrl_llc_action")

    def hrl_accum(self, rewards, dones, acc, first, last, llc_steps, terminate=None, logit=None, disc_scale=1.0, rewards_out=None,
                  disc_out=None, dones_out=None, terminate_out=None):
        """One inner step folded into acc f32 [4, n] (task-reward sum, discriminator-reward sum, done count, terminate count) and,
        with last, the finals (ase_hip_hrl_accum): rewards f32 [n]; dones / terminate [n] uint8 / bool / int32 / int64 / f32;
        logit f32 [n, ld] whose column 0 is the discriminator logit, read at its pitch; the four outputs f32 with n elements.
        Every tensor lives on the backend's device.  Recordable in a launch program."""
        n, f32 = dones.numel(), torch.float32
        vec = lambda t, dt, who: None if t is None else self._rs_vec(t, n, dt, who)
        rewards, dones, terminate = vec(rewards, f32, 'rewards'), vec(dones, None, 'dones'), vec(terminate, None, 'terminate')
        outs = [vec(t, f32, who) for t, who in ((rewards_out, 'rewards_out'), (disc_out, 'disc_out'), (dones_out, 'dones_out'),
                                                 (terminate_out, 'terminate_out'))]
        assert self._here(acc) and acc.dtype == f32 and acc.dim() == 2 and acc.shape == (4, n) and acc.stride(1) == 1 and \
            acc.stride(0) >= n, f"acc: f32 [4, {n}] rows on {self.device}"
        if logit is not None:
            assert self._here(logit) and logit.dtype == f32 and logit.dim() == 2 and logit.shape[0] == n and logit.stride(0) >= 1, \
                f"logit: f32 [{n}, ld] on {self.device}"
        kind = lambda t: 0 if t is None else self._KINDS[t.dtype]
        L.check(self.lib.ase_hip_hrl_accum(_ptr(rewards), _ptr(dones), kind(dones), _ptr(terminate), kind(terminate), _ptr(logit),
                                           _ld(logit), float(disc_scale), _ptr(acc), _ld(acc), int(bool(first)), int(bool(last)),
                                           int(llc_steps), *[_ptr(t) for t in outs], n, self._stream()), "hrl_accum")

    # ------------------------------------------------------------------ one environment step, one launch per side (N14)
    def _state_view(self, t, shape, who):
        """A state operand the step kernels read in place: f32 on this GPU, the last dimension dense, any environment / element
        stride that covers the elements (a contiguous tensor or a window of the simulator's packed tensor) -> (pointer,
        environment stride, element stride); a 2-d operand -> (pointer, row stride)."""
        assert self._here(t), f"{who}: a tensor on {self.device}, not {t.device}"
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(shape), f"{who}: f32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}"
        assert t.dim() == 2 or t.stride(2) == 1, f"{who}: the last dimension is dense"
        return _ptr(t), int(t.stride(0)), int(t.stride(1))      # (whether the strides cover the elements: the entry's own check)

    def _state_rows(self, t, n, cols, who):
        """[n, cols] rows with unit column stride at any row stride >= cols (an actor window of a packed tensor)."""
        if t is None:
            return None, 0
        assert self._here(t) and t.dtype == torch.float32 and tuple(t.shape) == (n, cols) and t.stride(1) == 1 and t.stride(0) >= cols, \
            f"{who}: f32 [{n}, {cols}] rows on {self.device}, unit column stride"
        return _ptr(t), int(t.stride(0))

    def _dense(self, t, numel, dtype, who):
        if t is None:
            return None
        assert self._here(t) and t.dtype == dtype and t.numel() == numel and t.is_contiguous(), \
            f"{who}: contiguous {dtype} of {numel} elements on {self.device}"
        return _ptr(t)

    def _id_array(self, ids):
        """The host-side id list of a body mask, built once per distinct list and kept."""
        if ids is None:
            return None, 0
        key = tuple(int(x) for x in ids)
        cache = self.__dict__.setdefault('_id_arrays', {})
        if key not in cache:
            cache[key] = (C.c_int32 * len(key))(*key)
        return cache[key], len(key)

    def env_pre_step(self, actions_in, actions, targets, clip_actions=1.0, pd_offset=None, pd_scale=None, motor_efforts=None,
                     power_scale=1.0, root_states=None, prev_root_pos=None, recovery_counter=None):
        """The pre_physics_step chain in one launch (ase_hip_env_pre_step): actions = clamp(actions_in, +-clip_actions) (actions_in
        f32 [n, D] at its own pitch, e.g. a view of the agent's buffer); targets = pd_offset + pd_scale * actions with pd_offset /
        pd_scale, else actions * motor_efforts * power_scale; prev_root_pos [n, 3] = root_states[:, 0:3] when given;
        recovery_counter int32 [n] = max(recovery_counter - 1, 0) when given.  Recordable in a launch program."""
        n, D = actions_in.shape
        f32 = torch.float32
        for t, who in ((actions_in, 'actions_in'), (actions, 'actions'), (targets, 'targets')):
            self._hrl_rows(t, n, D, f32, who)
        pd = pd_offset is not None
        assert pd == (pd_scale is not None) and pd != (motor_efforts is not None), "env_pre_step: pd_offset + pd_scale, or motor_efforts"
        rs, rs_stride = self._state_rows(root_states, n, 13, 'root_states')
        L.check(self.lib.ase_hip_env_pre_step(_ptr(actions_in), _ld(actions_in), float(clip_actions), _ptr(actions), _ld(actions),
                                              _ptr(targets), _ld(targets), int(pd), self._dense(pd_offset, D, f32, 'pd_offset'),
                                              self._dense(pd_scale, D, f32, 'pd_scale'), self._dense(motor_efforts, D, f32, 'motor_efforts'),
                                              float(power_scale), rs if prev_root_pos is not None else None, rs_stride,
                                              self._dense(prev_root_pos, 3 * n, f32, 'prev_root_pos'),
                                              self._dense(recovery_counter, n, torch.int32, 'recovery_counter'), n, D, self._stream()),
                "env_pre_step")

    def env_post_step(self, body_pos, body_rot, body_vel, body_ang_vel, contact_forces, progress_buf, obs, reward, reset, terminated,
                      termination_heights, contact_body_ids, max_episode_length, enable_early_termination, local_root_obs,
                      root_height_obs, col_offset=0, clip_obs=float('inf'), task_kind=None, enable_task_obs=True, task_col_offset=None,
                      root_states=None, prev_root_pos=None, tar_a=None, tar_b=None, tar_speed=None, tar_states=None, reach_body_id=0,
                      dt=0.0, tar_contact_forces=None, strike_body_ids=None, recovery_counter=None, hist=None, dof_pos=None,
                      dof_vel=None, dof_offsets=None, key_body_ids=None):
        """Humanoid.post_physics_step + HumanoidAMP.post_physics_step in one launch (ase_hip_env_post_step) on state read in place:
        body_pos / _vel / _ang_vel [n, B, 3], body_rot [n, B, 4], contact_forces [n, B, 3] and dof_pos / dof_vel [n, D] at any
        strides that cover them (windows of the simulator's packed tensors); root_states / tar_states [n, 13] and
        tar_contact_forces [n, 3] at any row stride.  progress_buf += 1; the humanoid columns at col_offset of obs and the task's
        at task_col_offset (default: right behind), clamped to +-clip_obs; reward (the task's, or 1); reset / terminated with
        the recovery mask when recovery_counter is given; hist [n, S, F] shifted and its slot 0 rebuilt when given.  Task operands
        as task_obs / task_reward take them (tar_speed: tensor [n] for heading, python float for location).  Recordable."""
        n, B = body_pos.shape[0], body_pos.shape[1]
        f32, i64 = torch.float32, torch.int64
        views = [self._state_view(t, (n, B, w), who) for t, w, who in ((body_pos, 3, 'body_pos'), (body_rot, 4, 'body_rot'),
                                                                       (body_vel, 3, 'body_vel'), (body_ang_vel, 3, 'body_ang_vel'),
                                                                       (contact_forces, 3, 'contact_forces'))]
        D = 0
        if hist is not None:
            assert self._here(hist) and hist.dtype == f32 and hist.dim() == 3 and hist.shape[0] == n and hist.is_contiguous(), \
                f"hist: contiguous f32 [{n}, S, F] on {self.device}"
            D = int(dof_offsets[-1])
            views += [self._state_view(t, (n, D), who) for t, who in ((dof_pos, 'dof_pos'), (dof_vel, 'dof_vel'))]
            assert hist.shape[2] == 13 + 6 * (len(dof_offsets) - 1) + D + 3 * len(key_body_ids), "hist: the frame width of the character"
        else:
            views += [(None, 0, 0), (None, 0, 0)]
        self._hrl_rows(obs, n, 1, f32, 'obs')
        kind = -1 if task_kind is None else int(task_kind)
        task_obs = bool(enable_task_obs) and kind >= 0
        if task_col_offset is None:
            task_col_offset = int(col_offset) + 15 * B - 2
        assert obs.shape[1] >= max(int(col_offset) + 15 * B - 2, int(task_col_offset) + L.TASK_OBS_COLS[kind] if task_obs else 0), \
            "obs: the columns do not fit its width"
        speed_t = tar_speed if torch.is_tensor(tar_speed) else None
        rs, rs_stride = self._state_rows(root_states, n, 13, 'root_states')
        ts, ts_stride = self._state_rows(tar_states, n, 13, 'tar_states')
        tc, tc_stride = self._state_rows(tar_contact_forces, n, 3, 'tar_contact_forces')
        wa = 3 if kind == L.TASK_REACH else 2
        offs, n_off = self._id_array(dof_offsets if hist is not None else None)
        keys, n_key = self._id_array(key_body_ids if hist is not None else None)
        contact, n_contact = self._id_array(contact_body_ids)
        strike, n_strike = self._id_array(strike_body_ids)
        L.check(self.lib.ase_hip_env_post_step(
            *[x for v in views for x in v], n, B, D, int(local_root_obs), int(root_height_obs), _ptr(obs), _ld(obs), int(col_offset),
            float(clip_obs), kind, int(task_obs), int(task_col_offset), rs, rs_stride, self._dense(prev_root_pos, 3 * n, f32, 'prev_root_pos'),
            self._dense(tar_a, wa * n, f32, 'tar_a'), self._dense(tar_b, 2 * n, f32, 'tar_b'), self._dense(speed_t, n, f32, 'tar_speed'),
            0.0 if speed_t is not None or tar_speed is None else float(tar_speed), ts, ts_stride, int(reach_body_id), float(dt),
            self._dense(reward, n, f32, 'reward'), self._dense(progress_buf, n, i64, 'progress_buf'),
            self._dense(termination_heights, B, f32, 'termination_heights'), contact, n_contact, tc, tc_stride, strike, n_strike,
            float(max_episode_length), int(enable_early_termination), self._dense(recovery_counter, n, torch.int32, 'recovery_counter'),
            self._dense(reset, n, i64, 'reset'), self._dense(terminated, n, i64, 'terminated'), _ptr(hist),
            0 if hist is None else hist.shape[1], offs, max(n_off - 1, 0), keys, n_key, self._stream()), "env_post_step")

    # ------------------------------------------------------------------ normaliser / gather
    def rms_moments(self, src, D, idx, remap, M, state, sums):
        L.check(self.lib.ase_hip_rms_moments(_ptr(src), _ld(src), D, _ptr(idx), remap[0], remap[1], M, _ptr(state),
                                             _ptr(sums), self._stream()), "rms_moments")

    @staticmethod
    def _stream_arrays(streams):
        n = len(streams)
        srcs = (C.c_void_p * n)(*[s[0].data_ptr() for s in streams])
        lds = (C.c_int64 * n)(*[int(s[0].stride(0)) for s in streams])
        idxs = (C.c_void_p * n)(*[None if s[1] is None else s[1].data_ptr() for s in streams])
        rh = (C.c_int * n)(*[int(s[2][0]) for s in streams])
        rn = (C.c_int * n)(*[int(s[2][1]) for s in streams])
        return n, srcs, lds, idxs, rh, rn

    def rms_moments_multi(self, streams, D, M, state, sums_list):
        """streams: [(src, idx, remap)] (<= 4, same width D and row count M); sums_list: one f64 [2 D] buffer per stream."""
        n, srcs, lds, idxs, rh, rn = self._stream_arrays(streams)
        sums = (C.c_void_p * n)(*[t.data_ptr() for t in sums_list])
        L.check(self.lib.ase_hip_rms_moments_multi(srcs, lds, idxs, rh, rn, sums, n, D, M, _ptr(state), self._stream()),
                "rms_moments_multi")

    def rms_normalize_multi(self, streams, D, M, means, stds, outs):
        n, srcs, lds, idxs, rh, rn = self._stream_arrays(streams)
        mp = (C.c_void_p * n)(*[t.data_ptr() for t in means])
        sp = (C.c_void_p * n)(*[t.data_ptr() for t in stds])
        op = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
        lo = (C.c_int64 * n)(*[int(t.stride(0)) for t in outs])
        L.check(self.lib.ase_hip_rms_normalize_multi(srcs, lds, idxs, rh, rn, mp, sp, op, lo, n, D, M, _code(outs[0].dtype),
                                                     self._stream()), "rms_normalize_multi")

    def rms_normalize_multi_twin(self, streams, D, M, means, stds, outs, outs32):
        """rms_normalize_multi with an f32 twin per stream (outs32: a tensor or None each): the normalised value before rounding."""
        n, srcs, lds, idxs, rh, rn = self._stream_arrays(streams)
        mp = (C.c_void_p * n)(*[t.data_ptr() for t in means])
        sp = (C.c_void_p * n)(*[t.data_ptr() for t in stds])
        op = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
        lo = (C.c_int64 * n)(*[int(t.stride(0)) for t in outs])
        assert all(t is None or t.dtype == torch.float32 for t in outs32)
        op32 = (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in outs32])
        lo32 = (C.c_int64 * n)(*[0 if t is None else int(t.stride(0)) for t in outs32])
        L.check(self.lib.ase_hip_rms_normalize_multi_v2(srcs, lds, idxs, rh, rn, mp, sp, op, lo, op32, lo32, n, D, M,
                                                        _code(outs[0].dtype), self._stream()), "rms_normalize_multi_v2")

    def rms_finalize(self, state, D, sums, count, n_streams, mean_out, std_out):
        counts = (C.c_int32 * max(n_streams, 1))(*([int(count)] * max(n_streams, 1)))
        L.check(self.lib.ase_hip_rms_finalize(_ptr(state), D, _ptr(sums), counts, n_streams, _ptr(mean_out),
                                              _ptr(std_out), self._stream()), "rms_finalize")

    def rms_normalize(self, src, D, idx, remap, M, mean, std, outs):
        outs = list(outs) + [None] * (3 - len(outs))
        dt = _code(outs[0].dtype)
        L.check(self.lib.ase_hip_rms_normalize(_ptr(src), _ld(src), D, _ptr(idx), remap[0], remap[1], M, _ptr(mean),
                                               _ptr(std), _ptr(outs[0]), _ld(outs[0]), _ptr(outs[1]), _ld(outs[1]),
                                               _ptr(outs[2]), _ld(outs[2]), dt, self._stream()), "rms_normalize")

    def rms_unnormalize(self, state, x, y):
        L.check(self.lib.ase_hip_rms_unnormalize(_ptr(state), _ptr(x), _ptr(y), x.numel(), self._stream()),
                "rms_unnormalize")

    def gather_rows(self, src, D, idx, remap, M, dst):
        L.check(self.lib.ase_hip_gather_rows(_ptr(src), _ld(src), D, _ptr(idx), remap[0], remap[1], M, _ptr(dst),
                                             _ld(dst), _code(dst.dtype), self._stream()), "gather_rows")

    # ------------------------------------------------------------------ heads
    def reduce_sum(self, x, n, square, acc, slot):
        L.check(self.lib.ase_hip_reduce_sum(_ptr(x), n, int(square), _ptr(acc), slot, self._stream()), "reduce_sum")

    def ppo_head(self, mu, value, mb, new_z, logstd, d_mu, d_value, db_mu, db_value, acc, M, m_global, act_dim,
                 z_dim, masked, div_on, mu_tanh, clip_value, e_clip, critic_coef, bounds_coef, div_coef, div_tar,
                 mu_out=None, grad_scale=1.0, dyn=None, ls_mode=L.LS_FROZEN, d_logstd=None, db_logstd=None, entropy_coef=0.0):
        """ls_mode (L.LS_*): LS_FROZEN - logstd f32[act_dim], no log-std gradient (the defaults reproduce the frozen call);
        LS_VECTOR - logstd f32[act_dim] learned; LS_ROWS - logstd f32[rows, >= act_dim] (a strided view, e.g. the sigma
        columns of the stacked head output).  Learned modes: d_logstd (nullable, d_mu's dtype) receives the per-row
        d loss / d logstd times grad_scale, db_logstd (nullable, f32[act_dim]) += its column sums."""
        scratch = self._head_scratch if ls_mode == L.LS_FROZEN else self.reserve_learned_logstd()
        L.check(self.lib.ase_hip_ppo_head(
            _ptr(mu), _ld(mu), _ptr(value), _ld(value), _ptr(mb['actions']), _ptr(mb['mu']), _ptr(mb['sigma']),
            _ptr(mb['old_logp_actions']), _ptr(mb['advantages']), _ptr(mb.get('old_values')), _ptr(mb['returns']),
            _ptr(mb.get('rand_action_mask')), _ptr(mb.get('ase_latents')), _ptr(new_z), _ptr(logstd),
            _ptr(d_mu), _ld(d_mu), _ptr(d_value), _ld(d_value), _ptr(db_mu), _ptr(db_value), _ptr(mu_out), _ptr(acc),
            _ptr(scratch),
            M, m_global, act_dim, z_dim, int(masked), int(div_on), int(mu_tanh), int(clip_value),
            float(e_clip), float(critic_coef), float(bounds_coef), float(div_coef), float(div_tar), float(grad_scale),
            _ptr(dyn), int(ls_mode), _ld(logstd) if ls_mode == L.LS_ROWS else 0, _ptr(d_logstd), _ld(d_logstd),
            _ptr(db_logstd), float(entropy_coef), _code(d_mu.dtype), self._stream()), "ppo_head")

    def reserve_learned_logstd(self):
        """The wider workspace of ppo_head's learned log-std modes (allocated once, before any launch program is recorded)."""
        if self._head_scratch_ls is None:
            self._head_scratch_ls = torch.zeros(L.PPO_SCRATCH_LS, dtype=torch.float64, device=self.device)
        return self._head_scratch_ls

    def disc_head(self, logit, d_logit, db_logit, acc, amb, amb_global, disc_coef, grad_scale=1.0, dyn=None, gp_add=None):
        """gp_add (nt_stack): an f64 cell added into acc[ACC_GP] by this launch (the stacked penalty schedule's sum of squares)."""
        assert gp_add is None or gp_add.dtype == torch.float64
        L.check(self.lib.ase_hip_disc_head_v2(_ptr(logit), _ld(logit), _ptr(d_logit), _ld(d_logit), _ptr(db_logit),
                                              _ptr(acc), amb, amb_global, float(disc_coef), float(grad_scale), _ptr(dyn),
                                              _ptr(gp_add), _code(d_logit.dtype), self._stream()), "disc_head")

    def enc_head(self, e, z, d_e, db_enc, enc_out, acc, amb, amb_global, z_dim, enc_coef, grad_scale=1.0, dyn=None):
        L.check(self.lib.ase_hip_enc_head(_ptr(e), _ld(e), _ptr(z), _ld(z), _ptr(d_e), _ld(d_e), _ptr(db_enc),
                                          _ptr(enc_out), _ptr(acc), amb, amb_global, z_dim, float(enc_coef), float(grad_scale),
                                          _ptr(dyn), _code(d_e.dtype), self._stream()), "enc_head")

    def enc_gp_seed(self, e, z, u, rows, z_dim, scale=1.0):
        """u[:rows, :z_dim] = scale * d enc_err / d e (learning/ase_agent.py:431-434; e f32 pre-normalisation output)."""
        assert e.dtype == torch.float32 and z.dtype == torch.float32
        L.check(self.lib.ase_hip_enc_gp_seed(_ptr(e), _ld(e), _ptr(z), _ld(z), _ptr(u), _ld(u), rows, z_dim, float(scale),
                                             _code(u.dtype), self._stream()), "enc_gp_seed")

    def enc_gp_back(self, e, z, du, d_e, db_enc, rows, z_dim, grad_scale=1.0, dyn=None):
        """d_e[:rows, :z_dim] += (d u / d e) du, the bias gradient follows the stored values."""
        assert e.dtype == torch.float32 and z.dtype == torch.float32 and du.dtype == torch.float32
        L.check(self.lib.ase_hip_enc_gp_back(_ptr(e), _ld(e), _ptr(z), _ld(z), _ptr(du), _ld(du), _ptr(d_e), _ld(d_e),
                                             _ptr(db_enc), rows, z_dim, float(grad_scale), _ptr(dyn), _code(d_e.dtype),
                                             self._stream()), "enc_gp_back")

    def gp_seed(self, h, w, g, rows, width, scale=1.0, act=L.ACT_RELU):
        L.check(self.lib.ase_hip_gp_seed(_ptr(h), _ld(h), _ptr(w), _ptr(g), _ld(g), rows, width, float(scale), int(act),
                                         _code(h.dtype), self._stream()), "gp_seed")

    def gp_second(self, twin, g, dg, dz, rows, width, act):
        """dz += act'' / act'^2 * g * dg (second-order term of the gradient penalty's backward, smooth activations)."""
        L.check(self.lib.ase_hip_gp_second(_ptr(twin), _ld(twin), _ptr(g), _ld(g), _ptr(dg), _ld(dg), _ptr(dz), _ld(dz), rows,
                                           width, int(act), _code(dz.dtype), self._stream()), "gp_second")

    def colsum(self, x, rows, cols, out, scale=1.0):
        assert x.dtype == torch.float32 and out.dtype == torch.float32
        L.check(self.lib.ase_hip_colsum(_ptr(x), _ld(x), rows, cols, float(scale), _ptr(out), self._stream()), "colsum")

    def sqnorm(self, x, rows, cols, acc, slot, scale=1.0, dyn=None):
        L.check(self.lib.ase_hip_sqnorm(_ptr(x), _ld(x), rows, cols, _ptr(acc), slot, float(scale), _ptr(dyn), _code(x.dtype),
                                        self._stream()),
                "sqnorm")

    def finalize_scalars(self, acc, out, m_global, amb_global, masked, has_disc, has_enc, has_div, c, opt_state=None, kl_threshold=0.0):
        L.check(self.lib.ase_hip_finalize_scalars(
            _ptr(acc), _ptr(out), m_global, amb_global, int(masked), int(has_disc), int(has_enc), int(has_div),
            float(c['critic_coef']), float(c['entropy_coef']), float(c.get('bounds_loss_coef') or 0.0), float(c.get('disc_coef', 0)),
            float(c.get('disc_logit_reg', 0)), float(c.get('disc_grad_penalty', 0)), float(c.get('disc_weight_decay', 0)),
            float(c.get('enc_coef', 0)), float(c.get('enc_weight_decay', 0)), float(c.get('amp_diversity_bonus', 0)),
            float(c.get('enc_grad_penalty', 0)), _ptr(opt_state), float(kl_threshold), self._stream()), "finalize_scalars")

    # ------------------------------------------------------------------ optimizer
    def begin_step(self, opt_state, acc, zero2=None, rng_bump=None):
        L.check(self.lib.ase_hip_begin_step(_ptr(opt_state), _ptr(acc), 0 if acc is None else acc.numel(), _ptr(zero2),
                                            0 if zero2 is None else zero2.numel(), _ptr(rng_bump), self._stream()),
                "begin_step")

    def adam(self, w, g, m, v, opt_state):
        L.check(self.lib.ase_hip_adam(_ptr(w), _ptr(g), _ptr(m), _ptr(v), w.numel(), _ptr(opt_state), self._stream()),
                "adam")

    def clip_scale(self, g, acc, slot, max_norm):
        L.check(self.lib.ase_hip_clip_scale(_ptr(g), g.numel(), _ptr(acc[slot:]), float(max_norm), self._stream()), "clip_scale")

    def axpy(self, g, w, c):
        L.check(self.lib.ase_hip_axpy(_ptr(g), _ptr(w), g.numel(), float(c), self._stream()), "axpy")

    def scaler_check(self, buf, scaler):
        """GradScaler's found_inf test over one buffer of the scaled backward (any view of contiguous storage)."""
        assert buf.is_contiguous()
        L.check(self.lib.ase_hip_scaler_check(_ptr(buf), buf.numel(), _code(buf.dtype), _ptr(scaler), self._stream()),
                "scaler_check")

    def scaler_check_multi(self, bufs, scaler, table=None):
        """The same test over a list of buffers in ONE launch; `table` = what make_check_table(bufs) returned (built once)."""
        if table is None:
            table = self.make_check_table(bufs)
        L.check(self.lib.ase_hip_scaler_check_multi(_ptr(table['rows']), table['n'], table['wg'], _ptr(scaler), self._stream()),
                "scaler_check_multi")

    def make_check_table(self, bufs):
        rows = []
        for t in bufs:
            assert t.is_contiguous() and t.numel() > 0
            rows.append([t.data_ptr(), t.numel(), _code(t.dtype)])
        big = max(t.numel() * t.element_size() for t in bufs)
        wg = max(1, min(1024, (big + 16383) // 16384))             # four 16-byte loads per thread of the largest buffer
        return {'rows': torch.tensor(rows, dtype=torch.int64, device=self.device), 'n': len(rows), 'wg': int(wg), 'keep': list(bufs)}

    def scaler_fold(self, scaler, scale_tab):
        """Overflow counts of the scale records -> scaler[found] (in front of the ranks' exchange of that flag)."""
        L.check(self.lib.ase_hip_scaler_fold(_ptr(scaler), _ptr(scale_tab), self._stream()), "scaler_fold")

    def scaler_step(self, scaler, opt_state, opt_eff, grads, scale_tab=None):
        """GradScaler.step's decision - a found overflow zeroes the gradient and hands the optimizer launch the identity step - and
        (scale_tab given) GradScaler.update(): backoff / growth of the device-resident scale and its table, every step."""
        L.check(self.lib.ase_hip_scaler_step(_ptr(scaler), _ptr(opt_state), _ptr(opt_eff), _ptr(grads), grads.numel(),
                                             _ptr(scale_tab), self._stream()), "scaler_step")

    # ------------------------------------------------------------------ rollout tail
    def disc_reward(self, logit, r, n, scale):
        L.check(self.lib.ase_hip_disc_reward(_ptr(logit), _ld(logit), _ptr(r), n, float(scale), self._stream()),
                "disc_reward")

    def enc_reward(self, e, z, r, n, z_dim, scale):
        L.check(self.lib.ase_hip_enc_reward(_ptr(e), _ld(e), _ptr(z), _ld(z), _ptr(r), n, z_dim, float(scale),
                                            self._stream()), "enc_reward")

    def gae(self, dones, values, next_values, r_task, r_disc, r_enc, w_task, w_disc, w_enc, gamma, tau, advs, returns,
            H, N):
        L.check(self.lib.ase_hip_gae(_ptr(dones), _ptr(values), _ptr(next_values), _ptr(r_task), _ptr(r_disc),
                                     _ptr(r_enc), float(w_task), float(w_disc), float(w_enc), float(gamma), float(tau),
                                     _ptr(advs), _ptr(returns), H, N, self._stream()), "gae")

    def adv_norm(self, returns, values, mask, adv, acc3, n, normalize, phase):
        L.check(self.lib.ase_hip_adv_norm(_ptr(returns), _ptr(values), _ptr(mask), _ptr(adv), _ptr(acc3), n,
                                          int(normalize), phase, self._stream()), "adv_norm")

    def ring_store(self, src, D, idx, remap, n, dst, size, head):
        L.check(self.lib.ase_hip_ring_store(_ptr(src), _ld(src), D, _ptr(idx), remap[0], remap[1], n, _ptr(dst), size,
                                            head, self._stream()), "ring_store")

    def normalize_rows(self, x, y, n, dim):
        L.check(self.lib.ase_hip_normalize_rows(_ptr(x), _ld(x), _ptr(y), _ld(y), n, dim, self._stream()), "normalize_rows")

    def sample_actions(self, mu, logstd, rand_probs, rng_state, mu_out, sigma_out, actions, neglogp, rand_mask, n, act_dim,
                       mu_tanh=False, logstd_rows=False):
        """logstd_rows: logstd is a per-row [n, >= act_dim] view (the sigma head's output) instead of one f32[act_dim] vector."""
        L.check(self.lib.ase_hip_sample_actions(_ptr(mu), _ld(mu), _ptr(logstd), _ld(logstd) if logstd_rows else 0,
                                                _ptr(rand_probs), _ptr(rng_state), _ptr(mu_out),
                                                _ptr(sigma_out), _ptr(actions), _ptr(neglogp), _ptr(rand_mask), n, act_dim,
                                                int(mu_tanh), self._stream()), "sample_actions")

    def sample_latents(self, z, rows, dim, rng_state, row_offset=0, advance=True, z2=None):
        L.check(self.lib.ase_hip_sample_latents(_ptr(z), rows, dim, _ptr(rng_state), int(row_offset), int(advance), _ptr(z2),
                                                _ld(z2), _code(z2.dtype) if z2 is not None else 0, self._stream()),
                "sample_latents")
