"""CPU stand-in of the retargeting launches (``ase_hip_retarget_*``, csrc/retarget.hip): the ``retarget_*`` methods
of ``HipBackend`` with the same signatures on CPU tensors, so that ``ase_amd.retarget.Retargeter`` - its name matching, its
integer tables, trimming and clip bookkeeping - runs under ``-m "not gpu"``.  It is TABLE-driven like the kernels (tree tables,
frame maps, roles), f64, and rounds to f32 where they do; tests/ref_retarget.py is the independent statement of what the
result has to be.  ``clip_frames`` / ``motion_state`` come from the clip loader's emulator, so a ``DeviceMotionLib`` loads the
retargeted clips."""
import numpy as np
import torch

from tests.emu_motion_load import EmuMotionLoad, quat_conjugate, quat_mul, quat_normalize, quat_rotate

# scipy.ndimage._gaussian_kernel1d(2, 0, 8)[8:], the literals of csrc/retarget.hip
GAUSS = (0.199474647864745, 0.17603575888479034, 0.12098748976534904, 0.06475993660472744, 0.026995957967298846,
         0.00876430436278587, 0.002215963172596555, 0.0004363490205067883, 6.691628957263553e-05)


def _qmn(a, b):
    return quat_normalize(quat_mul(a, b))


def _chain(tree, b):
    d = int(tree[b, 0])
    return [int(k) for k in tree[b, 1:d + 2]]


def _src_rows(clip_first, clip_num_frames, src_first, frame_clip):
    c = frame_clip.long()
    f = torch.arange(frame_clip.numel()) - clip_first.long()[c]
    assert bool(((f >= 0) & (f < clip_num_frames.long()[c])).all())
    return src_first.long()[c] + f


def _from_angle_axis(angle, axis):
    half = (angle / 2.0).unsqueeze(-1)
    axis = axis / axis.norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
    return quat_normalize(torch.cat([axis * half.sin(), half.cos()], dim=-1))


def _fk(tree, b, lr, lt, root):
    gr = gt = None
    for d, k in enumerate(_chain(tree, b)):
        l = root if k == 0 else lt[k].double().expand(lr.shape[0], 3)
        if d == 0:
            gr, gt = lr[:, k], l
        else:
            gt = quat_rotate(gr, l) + gt
            gr = _qmn(gr, lr[:, k])
    return gr, gt


class EmuRetarget(EmuMotionLoad):
    name = 'emu-retarget'

    def __init__(self):
        self.launches = []

    def _done(self, name, out, res):
        self.launches.append(name)
        res = res if isinstance(res, tuple) else (res,)
        if out is not None:
            out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
            for o, r in zip(out, res):
                o.copy_(r)
            res = out
        return res if len(res) > 1 else res[0]

    def retarget_fk(self, rotation, mode, tree, clip_first, clip_num_frames, src_first, frame_clip, out=None):
        assert rotation.dtype == torch.float64 and tree.dtype == torch.int32
        q = rotation[_src_rows(clip_first, clip_num_frames, src_first, frame_clip)]
        if mode == 1:
            return self._done('retarget_fk', out, q.clone())
        g = []
        for b in range(q.shape[1]):
            chain = _chain(tree, b)
            for d, k in enumerate(chain):
                l = q[:, k] if (mode == 0 or d == 0) else _qmn(quat_conjugate(q[:, chain[d - 1]]), q[:, k])
                acc = l if d == 0 else _qmn(acc, l)
            g.append(acc)
        return self._done('retarget_fk', out, torch.stack(g, dim=1))

    def retarget_chain(self, src_global, rs_body, rs_parent, rt_src, rt_tree, params, out=None):
        R = params[:4]
        g = []
        for i in range(rs_body.numel()):
            for d, k in enumerate(_chain(rt_tree, i)):
                m = int(rt_src[k])
                l = src_global[:, int(rs_body[m])]
                if int(rs_parent[m]) >= 0:
                    l = _qmn(quat_conjugate(src_global[:, int(rs_body[int(rs_parent[m])])]), l)
                if k == 0:
                    l = _qmn(R, l)
                acc = l if d == 0 else _qmn(acc, l)
            g.append(acc)
        return self._done('retarget_chain', out, torch.stack(g, dim=1))

    def retarget_pose(self, state_global, tpose_global, target_global, root_translation, params, rt_body, ancestor, parent_indices,
                      clip_first, clip_num_frames, src_first, frame_clip, out=None):
        R, src_root, tgt_root, scale = params[:4], params[4:7], params[7:10], params[10]
        new = _qmn(_qmn(state_global, quat_conjugate(tpose_global)), target_global[rt_body.long()])
        g = new[:, ancestor.long()]
        lr = torch.stack([g[:, b] if int(p) < 0 else _qmn(quat_conjugate(g[:, int(p)]), g[:, b])
                          for b, p in enumerate(parent_indices)], dim=1)
        root = root_translation[_src_rows(clip_first, clip_num_frames, src_first, frame_clip)]
        rt = tgt_root + (quat_rotate(R, root) - quat_rotate(R, src_root)) * scale
        return self._done('retarget_pose', out, (lr, rt))

    def retarget_hinge(self, local_rotation, root_translation, local_translation, tree, roles, out=None):
        lr, lt = local_rotation, local_translation
        new = lr.clone()
        y = torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float64)
        for b in range(lr.shape[1]):
            role, u, l, e, bend, sense = (int(x) for x in roles[b])
            if role == 0:
                continue
            if role == 1:
                new[:, b] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
                continue
            pu, pl, pe = (_fk(tree, k, lr, lt, root_translation)[1] for k in (u, l, e))
            d0, d1 = pu - pl, pe - pl
            d0 = d0 / (d0 * d0).sum(-1, keepdim=True).sqrt()
            d1 = d1 / (d1 * d1).sum(-1, keepdim=True).sqrt()
            theta = (-d0 * d1).sum(-1).clamp(-1.0, 1.0).acos()
            hinge = _from_angle_axis(-theta.abs() if bend < 0 else theta.abs(), y)
            if role == 3:
                new[:, b] = hinge
                continue
            direction = lt[e].double()
            direction = (direction / (direction * direction).sum().sqrt()).unsqueeze(0)
            tile = direction.expand(lr.shape[0], 3)
            dir0, dir1 = quat_rotate(lr[:, l], tile), quat_rotate(hinge, tile)
            twist = (dir0 * dir1).sum(-1).clamp(-1.0, 1.0).acos()
            twist = torch.where(dir0[:, 1] <= 0 if sense < 0 else dir0[:, 1] >= 0, twist, -twist)
            new[:, b] = quat_mul(lr[:, u], _from_angle_axis(twist, direction))
        return self._done('retarget_hinge', out, new)

    def retarget_ground(self, local_rotation, root_translation, local_translation, tree, clip_first, clip_num_frames, out=None):
        z = torch.stack([_fk(tree, b, local_rotation, local_translation, root_translation)[1][:, 2]
                         for b in range(local_rotation.shape[1])], dim=1)
        low = torch.stack([z[int(f):int(f) + int(n)].min() for f, n in zip(clip_first, clip_num_frames)])
        return self._done('retarget_ground', out, low)

    def retarget_finish(self, local_rotation, root_translation, min_z, params, local_translation, tree, frame_clip, out=None):
        root = root_translation.clone()
        root[:, 2] = root[:, 2] + -min_z[frame_clip.long()] + params[11]
        both = [_fk(tree, b, local_rotation, local_translation, root) for b in range(local_rotation.shape[1])]
        gr, gt = torch.stack([x[0] for x in both], dim=1), torch.stack([x[1] for x in both], dim=1)
        return self._done('retarget_finish', out, (gr, gt, local_rotation.float(), root.float()))

    def retarget_velocity(self, global_rotation, global_translation, clip_first, clip_num_frames, clip_fps, frame_clip, out=None):
        vel, ang = torch.zeros_like(global_translation), torch.zeros_like(global_translation)
        for first, n, fps in zip(clip_first.tolist(), clip_num_frames.tolist(), clip_fps.tolist()):
            assert n >= 2
            dt = 1.0 / fps
            p, r = global_translation[first:first + n], global_rotation[first:first + n]
            grad = torch.empty_like(p)
            grad[1:-1] = (p[2:] - p[:-2]) / 2.0
            grad[0], grad[-1] = (p[1] - p[0]) / 1.0, (p[-1] - p[-2]) / 1.0
            d = _qmn(r[1:], quat_conjugate(r[:-1]))
            angle = (2.0 * (d[..., 3] * d[..., 3]) - 1.0).clamp(-1.0, 1.0).acos()
            axis = d[..., :3] / d[..., :3].norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
            w = torch.zeros_like(p)
            w[:-1] = axis * angle.unsqueeze(-1) / dt
            i = torch.arange(n)

            def smooth(x):
                acc = x * GAUSS[0]
                for k in range(8, 0, -1):
                    acc = acc + (x[(i - k).clamp(0, n - 1)] + x[(i + k).clamp(0, n - 1)]) * GAUSS[k]
                return acc
            vel[first:first + n], ang[first:first + n] = smooth(grad) / dt, smooth(w)
        return self._done('retarget_velocity', out, (vel.float(), ang.float()))


def run_case(g, backend, device, trims=None, clips=None, order=None):
    """A case of tests/golden/retarget.pt through ``Retargeter`` on ``backend`` -> the list of output clip dicts."""
    from ase_amd.retarget import AMP_HUMANOID_HINGES, Retargeter
    from tests.ref_retarget import case_poses
    source, target = case_poses(g)
    r = Retargeter(backend, device, source, target, g['joint_mapping'], g['rotation'], g['scale'],
                   root_height_offset=g['root_height_offset'], hinges=AMP_HUMANOID_HINGES if g['hinges'] else None)
    clips = g['clips'] if clips is None else clips
    trims = g['trims'] if trims is None else trims
    if order is not None:
        clips, trims = [clips[i] for i in order], [trims[i] for i in order]
    return r.retarget([dict(c, rotation=c['rotation'].numpy(), root_translation=c['root_translation'].numpy()) for c in clips],
                      trim=[tuple(t) for t in trims])
