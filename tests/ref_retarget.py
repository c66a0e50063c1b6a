"""The reference's retargeting pipeline restated in torch and numpy, dtype-generic - NOT the emulator of the kernels
(tests/emu_retarget.py): it works by joint NAME on one clip at a time, the way ``poselib/retarget_motion.py`` does, and knows
nothing of the device tables.  Evaluated in f32 it reproduces the reference's recorded outputs (tests/golden/retarget.pt);
evaluated in f64 it is what the kernels and the emulator are held to.

Expressions, in the reference tree: SkeletonState.retarget_to / _transfer_to / _remapped_to / local_rotation /
global_transformation (poselib/skeleton/skeleton3d.py:403-424,462-482,706-713,757-784,786-948), SkeletonTree.
drop_nodes_by_names (:212-259, the offsets left out), SkeletonMotion._compute_velocity / _compute_angular_velocity
(:1223-1246), project_joints and the trim / grounding of main() (poselib/retarget_motion.py:24-175,211-243), and scipy's
gaussian_filter1d, whose 17 taps are written out here.

``WRONG`` names single-term wrong restatements; ``pipeline(..., wrong=name)`` evaluates one, and the tests check that each of
them fails a bound.
"""
import os

import numpy as np
import torch

from tests.emu_motion_load import GOLDEN, quat_conjugate, quat_mul, quat_rotate, ulp_f32
from tests.emu_motion_load import quat_normalize as _quat_normalize

RETARGET_DIR = os.path.join(GOLDEN, 'retarget')
WRONG = ('divide_before_filter', 'filter_wraps', 'central_ends', 'rotation_on_the_right', 'scale_on_target_root',
         'source_tree_recompose', 'arm_bend_positive', 'min_over_all_clips')
STAGES = ('pose_rotation', 'pose_root', 'hinge_rotation', 'min_h', 'rotation', 'root_translation', 'global_velocity',
          'global_angular_velocity')
LIMBS = (('right_upper_arm', 'right_lower_arm', 'right_hand', -1, -1), ('left_upper_arm', 'left_lower_arm', 'left_hand', -1, -1),
         ('right_thigh', 'right_shin', 'right_foot', +1, +1), ('left_thigh', 'left_shin', 'left_foot', +1, +1))
IDENTITY = ('left_hand', 'right_hand')
RADIUS = 8


def load_fixture():
    return torch.load(os.path.join(GOLDEN, 'retarget.pt'), weights_only=False)


def gauss_weights():
    """gaussian_filter1d(sigma=2): exp(-x^2 / (2 sigma^2)) over x = -8 .. 8, normalised (f64) -> the taps x = 0 .. 8."""
    x = np.arange(-RADIUS, RADIUS + 1)
    phi = np.exp(-0.5 / 4.0 * x ** 2)
    return (phi / phi.sum())[RADIUS:]


W_LOG = None           # a list: every quat_pos operand's |w| is appended to it (the fixture conditions)


def quat_normalize(q):
    if W_LOG is not None:
        W_LOG.append(q[..., 3].abs().reshape(-1))
    return _quat_normalize(q)


def quat_mul_norm(a, b):
    return quat_normalize(quat_mul(a, b))


def quat_from_angle_axis(angle, axis):
    half = (angle / 2).unsqueeze(-1)
    axis = axis / axis.norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
    return quat_normalize(torch.cat([axis * half.sin(), half.cos()], dim=-1))


def fk_rotation(parents, local):
    g = []
    for b, p in enumerate(parents):
        g.append(local[..., b, :] if p == -1 else quat_mul_norm(g[p], local[..., b, :]))
    return torch.stack(g, dim=-2)


def fk(parents, local, offsets, root):
    """-> (global rotation, global translation): transform_mul down the tree; body 0's local translation is the root's."""
    lt = offsets.broadcast_to(local.shape[:-2] + offsets.shape).clone()
    lt[..., 0, :] = root
    gr, gt = [], []
    for b, p in enumerate(parents):
        if p == -1:
            gr.append(local[..., b, :])
            gt.append(lt[..., b, :])
        else:
            gt.append(quat_rotate(gr[p], lt[..., b, :]) + gt[p])
            gr.append(quat_mul_norm(gr[p], local[..., b, :]))
    return torch.stack(gr, dim=-2), torch.stack(gt, dim=-2)


def local_from_global(parents, g):
    out = torch.zeros_like(g)
    for b, p in enumerate(parents):
        out[..., b, :] = g[..., b, :] if p == -1 else quat_mul_norm(quat_conjugate(g[..., p, :]), g[..., b, :])
    return out


def reduced_tree(names, parents, keep):
    kept = [b for b, n in enumerate(names) if n in keep]
    new_parent = []
    for b in kept:
        p = parents[b]
        while p != -1 and names[p] not in keep:
            p = parents[p]
        new_parent.append(-1 if p == -1 else kept.index(p))
    return kept, new_parent


class Setup:
    """A retargeting problem by name: T-poses (``read_tpose`` dicts), mapping, rotation, scale, offset - cast to ``dtype``."""

    def __init__(self, source, target, mapping, rotation, scale, root_height_offset, hinges, dtype):
        t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)
        self.dtype, self.mapping, self.hinges = dtype, dict(mapping), hinges
        self.scale, self.offset = float(scale), float(root_height_offset)
        self.R = torch.tensor([float(x) for x in rotation], dtype=torch.float32).to(dtype)       # torch.tensor(json list): f32
        self.src_names, self.src_parents = list(source['node_names']), [int(p) for p in source['parent_indices']]
        self.tgt_names, self.tgt_parents = list(target['node_names']), [int(p) for p in target['parent_indices']]
        self.tgt_offsets = t(target['local_translation'])
        local = lambda s, parents: t(s['rotation']) if s['is_local'] else local_from_global(parents, t(s['rotation']))
        self.src_tpose_local, self.src_tpose_root = local(source, self.src_parents), t(source['root_translation'])
        self.tgt_tpose_local, self.tgt_tpose_root = local(target, self.tgt_parents), t(target['root_translation'])


def pose_transfer(S, rotation, root, is_local, wrong=None):
    """retarget_to_by_tpose -> (local rotation on the target tree [F, Bt, 4], root translation [F, 3])."""
    inv = {v: k for k, v in S.mapping.items()}
    rs, rs_parent = reduced_tree(S.src_names, S.src_parents, set(S.mapping))
    rt, rt_parent = reduced_tree(S.tgt_names, S.tgt_parents, set(inv))
    assert len(S.mapping) == len(rs) == len(rt)
    rs_names = [S.src_names[b] for b in rs]
    rt_names = [S.tgt_names[b] for b in rt]
    order = [rs_names.index(inv[n]) for n in rt_names]

    def remap(g_source, root_t):
        l = local_from_global(rs_parent, g_source[..., rs, :])
        if wrong == 'source_tree_recompose':
            l0 = l.clone()
            l0[..., 0, :] = quat_mul_norm(S.R, l[..., 0, :])
            return fk_rotation(rs_parent, l0)[..., order, :], quat_rotate(S.R, root_t)
        l = l[..., order, :]
        l0 = l.clone()
        l0[..., 0, :] = quat_mul_norm(l[..., 0, :], S.R) if wrong == 'rotation_on_the_right' else quat_mul_norm(S.R, l[..., 0, :])
        return fk_rotation(rt_parent, l0), quat_rotate(S.R, root_t)

    g_state, root_state = remap(fk_rotation(S.src_parents, rotation) if is_local else rotation, root)
    g_tpose, root_tpose = remap(fk_rotation(S.src_parents, S.src_tpose_local), S.src_tpose_root)
    root_diff = (root_state - root_tpose) * S.scale
    target_global = fk_rotation(S.tgt_parents, S.tgt_tpose_local)[[S.tgt_names.index(n) for n in rt_names]]
    new_global = quat_mul_norm(quat_mul_norm(g_state, quat_conjugate(g_tpose)), target_global)
    take = []
    for n in S.tgt_names:
        while n not in rt_names:
            n = S.tgt_names[S.tgt_parents[S.tgt_names.index(n)]]
        take.append(rt_names.index(n))
    out_global = torch.zeros(new_global.shape[:-2] + (len(S.tgt_names), 4), dtype=new_global.dtype)
    for b, i in enumerate(take):
        out_global[:, b, :] = new_global[:, i, :]
    S.last_global = out_global
    tgt_root = S.tgt_tpose_root * S.scale if wrong == 'scale_on_target_root' else S.tgt_tpose_root
    return local_from_global(S.tgt_parents, out_global), tgt_root + root_diff


def project_joints(S, local, root, wrong=None, record=None):
    """project_joints -> new local rotations.  ``record``: a dict that receives dir0.y / the bend sign per limb."""
    _, gt = fk(S.tgt_parents, local, S.tgt_offsets, root)
    idx = S.tgt_names.index
    new = local.clone()
    y_axis = torch.tensor([[0.0, 1.0, 0.0]], dtype=S.dtype)
    for upper, lower, end, bend, sense in S.hinges['limbs']:
        u, l, e = idx(upper), idx(lower), idx(end)
        d0, d1 = gt[..., u, :] - gt[..., l, :], gt[..., e, :] - gt[..., l, :]
        d0 = d0 / torch.norm(d0, dim=-1, keepdim=True)
        d1 = d1 / torch.norm(d1, dim=-1, keepdim=True)
        theta = torch.acos(torch.clamp(torch.sum(-d0 * d1, dim=-1), -1.0, 1.0))
        if wrong == 'arm_bend_positive' and bend < 0:
            bend = 1
        hinge = quat_from_angle_axis(torch.abs(theta) if bend > 0 else -torch.abs(theta), y_axis)
        direction = S.tgt_offsets[e] / torch.norm(S.tgt_offsets[e])
        tile = torch.tile(direction.unsqueeze(0), [local.shape[0], 1])
        dir0, dir1 = quat_rotate(local[..., l, :], tile), quat_rotate(hinge, tile)
        twist = torch.acos(torch.clamp(torch.sum(dir0 * dir1, dim=-1), -1.0, 1.0))
        twist = torch.where(dir0[..., 1] <= 0 if sense < 0 else dir0[..., 1] >= 0, twist, -twist)
        new[..., u, :] = quat_mul(local[..., u, :], quat_from_angle_axis(twist, direction.unsqueeze(0)))
        new[..., l, :] = hinge
        if record is not None:
            record[upper] = dir0[..., 1].clone()
    for n in S.hinges.get('identity', ()):
        new[..., idx(n), :] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=S.dtype)
    return new


def gradient(p, wrong=None):
    """numpy.gradient along axis 0, unit spacing: central differences, one-sided ends."""
    g = np.empty_like(p)
    g[1:-1] = (p[2:] - p[:-2]) / 2.0
    if wrong == 'central_ends':
        g[0], g[-1] = (p[1] - p[0]) / 2.0, (p[-1] - p[-2]) / 2.0
    else:
        g[0], g[-1] = (p[1] - p[0]) / 1.0, (p[-1] - p[-2]) / 1.0
    return g


def gauss_filter(x, wrong=None):
    """gaussian_filter1d(x, 2, axis=0, mode='nearest'): f64 accumulation in the order of scipy's symmetric correlation (centre
    tap, then the pairs from the outermost in), indices clamped to the array, the result cast to x's dtype."""
    w = gauss_weights()
    n = x.shape[0]
    x64 = x.astype(np.float64)
    i = np.arange(n)
    at = (lambda j: x64[j % n]) if wrong == 'filter_wraps' else (lambda j: x64[np.clip(j, 0, n - 1)])
    acc = x64 * w[0]
    for k in range(RADIUS, 0, -1):
        acc = acc + (at(i - k) + at(i + k)) * w[k]
    return acc.astype(x.dtype)


def velocities(gr, gt, fps, wrong=None):
    """from_skeleton_state -> (global velocity, global angular velocity)."""
    time_delta = 1 / fps
    p = gt.numpy()
    if wrong == 'divide_before_filter':
        vel = gauss_filter(gradient(p / time_delta))
    else:
        vel = gauss_filter(gradient(p, wrong), wrong) / time_delta
    d = torch.zeros_like(gr)
    d[..., 3] = 1.0
    d[:-1] = quat_mul_norm(gr[1:], quat_conjugate(gr[:-1]))
    angle = (2 * (d[..., 3] ** 2) - 1).clamp(-1, 1).arccos()
    axis = d[..., :3] / d[..., :3].norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
    ang = axis * angle.unsqueeze(-1) / time_delta
    return torch.from_numpy(np.ascontiguousarray(vel)), torch.from_numpy(gauss_filter(ang.numpy(), wrong))


def trim_range(frames, trim):
    beg, end = trim
    return (0 if beg == -1 else beg), (frames if end == -1 else min(end, frames))


def pipeline(S, clips, trims, wrong=None, record=None):
    """retarget_motion.main() for each clip -> list of dicts of STAGES.  clips: dicts with rotation, root_translation (any float
    dtype, cast to S.dtype), fps, is_local."""
    staged = []
    for clip, trim in zip(clips, trims):
        rot = torch.as_tensor(clip['rotation']).to(S.dtype)
        root = torch.as_tensor(clip['root_translation']).to(S.dtype)
        pose_rot, pose_root = pose_transfer(S, rot, root, clip.get('is_local', True), wrong)
        beg, end = trim_range(rot.shape[0], trim)
        local, root_t = pose_rot[beg:end], pose_root[beg:end].clone()
        rec = {} if record is not None else None
        hinge = project_joints(S, local, root_t, wrong, rec) if S.hinges is not None else local
        if record is not None:
            record.append(rec)
        _, gt = fk(S.tgt_parents, hinge, S.tgt_offsets, root_t)
        staged.append({'pose_rotation': pose_rot, 'pose_root': pose_root, 'hinge_rotation': hinge, 'min_h': torch.min(gt[..., 2]),
                       'root_t': root_t, 'fps': clip['fps']})
    if wrong == 'min_over_all_clips':
        low = torch.min(torch.stack([s['min_h'] for s in staged]))
        for s in staged:
            s['min_h'] = low
    out = []
    for s in staged:
        root_t = s.pop('root_t')
        root_t[:, 2] += -s['min_h']
        root_t[:, 2] += S.offset
        gr, gt = fk(S.tgt_parents, s['hinge_rotation'], S.tgt_offsets, root_t)
        vel, ang = velocities(gr, gt, s.pop('fps'), wrong)
        s.update(rotation=s['hinge_rotation'], root_translation=root_t, global_velocity=vel, global_angular_velocity=ang)
        out.append(s)
    return out


def bound(stage, ref, fps, hinges):
    """The GPU bounds of a stage's output against the f64 restatement ``ref``: one f32 rounding plus what libm's f64 sqrt /
    acos / sin / cos may differ by - 1e-12 where no angle passes a clamp, 6e-8 rad where the bend and twist angles (or the
    frame-to-frame angle of the angular velocity) go through acos next to its clamp: an argument error of 16 x 2^-53 moves the
    angle by at most sqrt(2 delta) = 6e-8.  The filter is a convex combination, so a bound carries through it; velocities
    divide by dt = 1 / fps."""
    slack = {'pose_rotation': 1e-12, 'pose_root': 1e-12, 'root_translation': 1e-12, 'min_h': 1e-12,
             'hinge_rotation': 6e-8 if hinges else 1e-12, 'rotation': 6e-8 if hinges else 1e-12,
             'global_velocity': 1e-12 * fps, 'global_angular_velocity': 6e-8 * fps}[stage]
    return ulp_f32(ref) + slack


def quat_error(got, ref):
    """|got - ref| of quaternion arrays [..., 4]; where the f64 reference has |w| < 1e-3 - quat_pos may have flipped either -
    the quaternion is compared up to one common sign.  -> (error, number of such quaternions)."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    loose = ref[..., 3].abs() < 1e-3
    flipped = (got + ref).abs()
    use = loose & (flipped.amax(-1) < err.amax(-1))
    return torch.where(use.unsqueeze(-1), flipped, err), int(loose.sum())


def case_poses(g):
    """The T-poses of a case of the fixture -> (source, target) in ``read_tpose``'s form.  The ``unmapped`` / ``topology``
    target is the tree of a committed clip in zero pose."""
    from ase_amd.motion_lib import read_clip
    from ase_amd.retarget import read_tpose, zero_pose
    source = read_tpose(os.path.join(RETARGET_DIR, g['source_tpose']))
    if g['target'].endswith('tpose.npy'):
        return source, read_tpose(os.path.join(RETARGET_DIR, g['target']))
    c = read_clip(os.path.join(GOLDEN, 'clips', g['target']))
    return source, zero_pose(c['node_names'], c['parent_indices'], c['local_translation'])


def case_setup(g, dtype):
    source, target = case_poses(g)
    hinges = {'limbs': LIMBS, 'identity': IDENTITY} if g['hinges'] else None
    return Setup(source, target, g['joint_mapping'], g['rotation'], g['scale'], g['root_height_offset'], hinges, dtype)
