"""Plain-torch f64 restatement of ``HipBackend.clip_frames`` (``ase_hip_clip_frames``, csrc/motion_load.hip) with
the same signature - the emulator of the clip loader - and the helpers the loader's tests share.

Follows the reference operation by operation: poselib/core/rotation3d.py (quat_mul :8-20, quat_normalize :24-49,88-93,
quat_rotate :201-206, quat_angle_axis :226-235, transform_mul :318-327), SkeletonState.global_transformation /
local_translation (poselib/skeleton/skeleton3d.py:403-424,495-510) and MotionLib._compute_motion_dof_vels /
_local_rotation_to_dof_vel (utils/motion_lib.py:279-294,326-355), vectorised over the frames of a clip.  On the CPU it is
bitwise equal to the reference's loader (tests/test_motion_load_emu.py), which isolates a device function when the kernel
differs."""
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CLIP_DIR = os.path.join(GOLDEN, 'clips')
ARRAYS = ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs')
TABLES = ('lengths', 'num_frames', 'dt', 'length_starts')
OUT_NAMES = ('root_pos', 'root_rot', 'dof_pos', 'root_vel', 'root_ang_vel', 'dof_vel', 'key_pos')


def quat_mul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
    x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2
    y = w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2
    z = w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2
    return torch.stack([x, y, z, w], dim=-1)


def quat_normalize(q):
    z = (q[..., 3:] < 0).float()
    q = (1 - 2 * z) * q
    return q / q.norm(p=2, dim=-1).unsqueeze(-1).clamp(min=1e-9)


def quat_conjugate(x):
    return torch.cat([-x[..., :3], x[..., 3:]], dim=-1)


def quat_rotate(rot, vec):
    other_q = torch.cat([vec, torch.zeros_like(vec[..., :1])], dim=-1)
    return quat_mul(quat_mul(rot, other_q), quat_conjugate(rot))[..., :3]


class EmuMotionLoad:
    """``clip_frames`` of HipBackend on CPU tensors (plus ``motion_state`` through the oracle restatement, so that a
    ``DeviceMotionLib`` loaded with this backend samples).  ``min_abs_w`` / ``zero_angles`` are kept from the last call: the
    smallest |w| any product had before it was normalised, and the number of frame pairs of a joint body with angle == 0."""
    name = 'emu-motion-load'

    def clip_frames(self, rotation, root_translation, root_velocity, root_angular_velocity, local_translation, parent_indices,
                    clip_first, clip_num_frames, clip_fps, frame_clip, dof_body_ids, dof_offsets, out=None):
        T, B = rotation.shape[0], rotation.shape[1]
        D = int(dof_offsets[-1])
        assert rotation.dtype == root_translation.dtype == clip_fps.dtype == torch.float64 and local_translation.dtype == torch.float32
        gts, grs = torch.zeros(T, B, 3, dtype=torch.float64), torch.zeros(T, B, 4, dtype=torch.float64)
        dvs = torch.zeros(T, D, dtype=torch.float32)
        self.min_abs_w, self.zero_angles = float('inf'), 0
        for c in range(clip_first.numel()):
            f0, n = int(clip_first[c]), int(clip_num_frames[c])
            assert torch.equal(frame_clip[f0:f0 + n], torch.full((n,), c, dtype=frame_clip.dtype))
            rot = rotation[f0:f0 + n]
            # SkeletonState.local_translation: the tree's f32 offsets, row 0 overwritten by the f64 root translation - the
            # assignment rounds it to f32; torch.cat with the f64 rotations then promotes
            lt = local_translation[c].broadcast_to(n, B, 3).clone()
            lt[:, 0] = root_translation[f0:f0 + n]
            lt = lt.double()
            g_rot, g_tr = [], []
            for b in range(B):
                p = int(parent_indices[b])
                if p == -1:
                    g_rot.append(rot[:, b])
                    g_tr.append(lt[:, b])
                else:
                    prod = quat_mul(g_rot[p], rot[:, b])
                    self.min_abs_w = min(self.min_abs_w, float(prod[..., 3].abs().min()))
                    g_tr.append(quat_rotate(g_rot[p], lt[:, b]) + g_tr[p])
                    g_rot.append(quat_normalize(prod))
            grs[f0:f0 + n], gts[f0:f0 + n] = torch.stack(g_rot, dim=1), torch.stack(g_tr, dim=1)
            # _local_rotation_to_dof_vel for the frame pairs (f, f + 1); the last frame repeats the one before
            dt = 1.0 / float(clip_fps[c])
            prod = quat_mul(quat_conjugate(rot[:-1]), rot[1:])
            d = quat_normalize(prod)
            angle = (2 * (d[..., 3] ** 2) - 1).clamp(-1, 1).arccos()
            axis = d[..., :3] / d[..., :3].norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
            vel = axis * angle.unsqueeze(-1) / dt
            bodies = [int(b) for b in dof_body_ids]
            self.min_abs_w = min(self.min_abs_w, float(prod[:, bodies, 3].abs().min()))
            self.zero_angles += int((angle[:, bodies] == 0).sum())
            for j, b in enumerate(bodies):
                off, size = int(dof_offsets[j]), int(dof_offsets[j + 1]) - int(dof_offsets[j])
                assert size in (1, 3)
                dvs[f0:f0 + n - 1, off:off + size] = vel[:, b] if size == 3 else vel[:, b, 1:2]      # (rounds to f32)
            dvs[f0 + n - 1] = dvs[f0 + n - 2]
        res = (gts.float(), grs.float(), rotation.float(), root_velocity.float(), root_angular_velocity.float(), dvs)
        if out is not None:
            for o, r in zip(out, res):
                o.copy_(r)
            return tuple(out)
        return res

    def motion_state(self, clips, motion_ids, times):
        from oracle import amp_obs as A
        c = dict(clips)
        for k in ('num_frames', 'length_starts'):
            c[k] = clips[k].long()
        return A.motion_state(c, motion_ids.long(), times)


def load_fixture():
    """tests/golden/motion_load.pt (scripts/make_golden_motion_load.py): cases 'a' (three.yaml) and 'b' (amp_humanoid_run.npy)."""
    return torch.load(os.path.join(GOLDEN, 'motion_load.pt'), weights_only=False)


def case_args(g):
    """The arguments of ``DeviceMotionLib.from_file`` for a case of the fixture."""
    return os.path.join(CLIP_DIR, g['motion_file']), g['dof_body_ids'], g['dof_offsets'], g['key_body_ids']


def golden_clips(g):
    """A case's recorded arrays and tables in the form ``DeviceMotionLib.from_arrays`` takes."""
    c = dict(g['clips'])
    c.update(dof_body_ids=g['dof_body_ids'], dof_offsets=g['dof_offsets'], key_body_ids=g['key_body_ids'])
    return c


def bits_equal(a, b):
    """Same shape, dtype and bit patterns (so -0.0 != 0.0 and NaN == NaN) -> number of elements compared."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    view = {torch.float32: torch.int32, torch.float64: torch.int64}.get(a.dtype)
    a, b = (a.contiguous().view(view), b.contiguous().view(view)) if view else (a, b)
    assert torch.equal(a, b), f'{int((a != b).sum())} of {a.numel()} elements differ'
    return a.numel()


def ulp_f32(x):
    """The spacing of f32 at |x| (f64 tensor), the smallest normal's spacing below it."""
    x = x.double().abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)
