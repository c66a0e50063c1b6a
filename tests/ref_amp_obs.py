"""Reference, fixtures and checks of the AMP observation and motion sampler kernels (COVERAGE row N2).  TEST INFRASTRUCTURE.

The reference's own expressions restated in torch, dtype-generic: one call runs in f32 (the reference as it runs) and one in f64
(the yardstick); e_ref = |f32 run - f64 run|.  NOT the emulator: nothing here imports oracle/amp_obs.py; tests/test_amp_obs_ref.py
holds that module to this one.  Every branch decision is returned beside the values, per row, so that the tests can assert
the margins of the fixtures and count the rows that reach each branch.

Bound, per group (one output tensor or column block, within one decision class):

    max |got - f64| <= 2 max e_ref + 2^-23 max |ref| + 1e-7 (+ max acos allowance)

Angles read back from acos(w) (``quat_to_angle_axis``): w reaches acos rounded to f32, half an ulp of a number below 1 is up to
2^-24, d(2 acos w)/dw = -2 / sin_theta, so the angle carries 2^-23 / sin_theta whichever way w was rounded; an output with
|d out / d angle| = |axis_c| (the exponential map) or |axis_y| (the hinge) carries that times the factor.  One f32 evaluation
(e_ref) shows one rounding of w, the device another, so the term is added to the bound (``acos_allowance``).

The length of an exponential map (``exp_map_to_angle_axis``): |e| = sqrt(x^2 + y^2 + z^2) carries three roundings of the squares'
sum (one per square at most, two additions), halved by the root, and the root's own: 2.5 x 2^-24 |e|.  The angle is |e| wrapped
into (-pi, pi], so it carries that ABSOLUTE error whatever the wrapped angle's size, and the tangent / normal of the joint turn
by it: |d out / d angle| <= 1 for a rotating unit vector.  2.5 x 2^-24 |e| is added for the six columns of every 3-dof joint that
does not take the default (``len_allowance``; 1.0e-6 at |e| = 7, where a single row's e_ref showed 5e-8 and the MI355X differed
from f64 by 4.5e-7: observed / allowed 0.33 with the term).
"""
import contextlib
import math

import torch

EPS23 = 2.0 ** -23
EPS24 = 2.0 ** -24
FLOOR = 1e-7
MARGIN = 1e-3                      # relative distance of every f32 decision variable from its threshold (tests/test_heads_ref.py)
STATS = {}                         # (op, output, group) -> [max |got - f64|, max e_ref, max err / allowed]
COUNTS = {'cases': 0, 'elements': 0, 'sentinels': 0}

_MUT = None
MUTATIONS = ('slerp_no_flip', 'slerp_mid_q0', 'blend_from_i1', 'i1_unclamped', 'root_vel_f1', 'hinge_z_dof', 'hinge_z_obs',
             'expmap_no_wrap', 'angle_axis_no_wrap', 'hinge_no_second_wrap', 'local_root_ignored', 'heading_not_inverted',
             'keys_not_relative', 'normal_from_y', 'hist_towards_present')


@contextlib.contextmanager
def mutated(name):
    """Run the reference with ONE term restated wrongly (tests/test_amp_obs_ref.py shows that each fails a bound)."""
    global _MUT
    assert name in MUTATIONS
    _MUT = name
    try:
        yield
    finally:
        _MUT = None


# ------------------------------------------------------------------------------------------------------------------------
# isaacgym.torch_utils as oracle/rl_games_shim/isaacgym/torch_utils.py states them
# ------------------------------------------------------------------------------------------------------------------------
def normalize(x, eps=1e-9):                                                   # shim :16-17
    return x / x.norm(p=2, dim=-1).clamp(min=eps, max=None).unsqueeze(-1)


def quat_mul(a, b):                                                           # shim :26-42
    shape = a.shape
    a, b = a.reshape(-1, 4), b.reshape(-1, 4)
    x1, y1, z1, w1 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    x2, y2, z2, w2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    w = qq - ww + (z1 - y1) * (y2 - z2)
    x = qq - xx + (x1 + w1) * (x2 + w2)
    y = qq - yy + (w1 - x1) * (y2 + z2)
    z = qq - zz + (z1 + y1) * (w2 - x2)
    return torch.stack([x, y, z, w], dim=-1).view(shape)


def quat_rotate(q, v):                                                        # shim :53-60
    shape = q.shape
    q_w = q[:, -1]
    q_vec = q[:, :3]
    a = v * (2.0 * q_w ** 2 - 1.0).unsqueeze(-1)
    b = torch.cross(q_vec, v, dim=-1) * q_w.unsqueeze(-1) * 2.0
    c = q_vec * torch.bmm(q_vec.reshape(shape[0], 1, 3), v.reshape(shape[0], 3, 1)).squeeze(-1) * 2.0
    return a + b + c


def quat_from_angle_axis(angle, axis):                                        # shim :75-79
    theta = (angle / 2).unsqueeze(-1)
    xyz = normalize(axis) * theta.sin()
    w = theta.cos()
    return normalize(torch.cat([xyz, w], dim=-1))


def normalize_angle(x):                                                       # shim :83-84
    return torch.atan2(torch.sin(x), torch.cos(x))


# ------------------------------------------------------------------------------------------------------------------------
# utils/torch_utils.py
# ------------------------------------------------------------------------------------------------------------------------
def quat_to_angle_axis(q):
    """utils/torch_utils.py:7-27.  Also returns the decision (mask) and its variable (sin_theta)."""
    min_theta = 1e-5
    sin_theta = torch.sqrt(1 - q[..., 3] * q[..., 3])
    angle = 2 * torch.acos(q[..., 3])
    if _MUT != 'angle_axis_no_wrap':
        angle = normalize_angle(angle)
    axis = q[..., 0:3] / sin_theta.unsqueeze(-1)
    mask = torch.abs(sin_theta) > min_theta
    default_axis = torch.zeros_like(axis)
    default_axis[..., -1] = 1
    angle = torch.where(mask, angle, torch.zeros_like(angle))
    axis = torch.where(mask.unsqueeze(-1), axis, default_axis)
    return angle, axis, mask, sin_theta


def quat_to_tan_norm(q):
    """utils/torch_utils.py:46-59."""
    ref_tan = torch.zeros_like(q[..., 0:3])
    ref_tan[..., 0] = 1
    tan = quat_rotate(q, ref_tan)
    ref_norm = torch.zeros_like(q[..., 0:3])
    ref_norm[..., 1 if _MUT == 'normal_from_y' else -1] = 1
    norm = quat_rotate(q, ref_norm)
    return torch.cat([tan, norm], dim=len(tan.shape) - 1)


def exp_map_to_quat(exp_map):
    """utils/torch_utils.py:69-91 (exp_map_to_angle_axis + exp_map_to_quat).  Also returns the mask and the wrapped angle."""
    min_theta = 1e-5
    angle = torch.norm(exp_map, dim=-1)
    axis = exp_map / torch.unsqueeze(angle, dim=-1)
    if _MUT != 'expmap_no_wrap':
        angle = normalize_angle(angle)
    default_axis = torch.zeros_like(exp_map)
    default_axis[..., -1] = 1
    mask = torch.abs(angle) > min_theta
    var = angle
    angle = torch.where(mask, angle, torch.zeros_like(angle))
    axis = torch.where(mask.unsqueeze(-1), axis, default_axis)
    return quat_from_angle_axis(angle, axis), mask, var


SLERP_GENERIC, SLERP_MID, SLERP_ONE = 0, 1, 2


def slerp(q0, q1, t):
    """utils/torch_utils.py:94-115.  Decisions: the sign flip, the class (generic / midpoint / q0) and their variables."""
    cos_half_theta = torch.sum(q0 * q1, dim=-1)
    neg_mask = cos_half_theta < 0
    signed = cos_half_theta
    q1 = q1.clone()
    if _MUT != 'slerp_no_flip':
        q1[neg_mask] = -q1[neg_mask]
    cos_half_theta = torch.abs(cos_half_theta)
    cos_half_theta = torch.unsqueeze(cos_half_theta, dim=-1)
    half_theta = torch.acos(cos_half_theta)
    sin_half_theta = torch.sqrt(1.0 - cos_half_theta * cos_half_theta)
    ratioA = torch.sin((1 - t) * half_theta) / sin_half_theta
    ratioB = torch.sin(t * half_theta) / sin_half_theta
    new_q = ratioA * q0 + ratioB * q1
    mid = torch.abs(sin_half_theta) < 0.001
    one = torch.abs(cos_half_theta) >= 1
    new_q = torch.where(mid, q0 + 0 * q1 if _MUT == 'slerp_mid_q0' else 0.5 * q0 + 0.5 * q1, new_q)
    new_q = torch.where(one, q0, new_q)
    cls = torch.where(one, SLERP_ONE, torch.where(mid, SLERP_MID, SLERP_GENERIC)).squeeze(-1)
    return new_q, {'flip': neg_mask, 'cls': cls, 'c': signed, 's': sin_half_theta.squeeze(-1)}


def calc_heading_quat_inv(q):
    """utils/torch_utils.py:118-154 (calc_heading + calc_heading_quat_inv).  Also returns the rotated x axis."""
    ref_dir = torch.zeros_like(q[..., 0:3])
    ref_dir[..., 0] = 1
    rot_dir = quat_rotate(q, ref_dir)
    heading = torch.atan2(rot_dir[..., 1], rot_dir[..., 0])
    axis = torch.zeros_like(q[..., 0:3])
    axis[..., 2] = 1
    return quat_from_angle_axis(heading if _MUT == 'heading_not_inverted' else -heading, axis), rot_dir


# ------------------------------------------------------------------------------------------------------------------------
# utils/motion_lib.py
# ------------------------------------------------------------------------------------------------------------------------
def calc_frame_blend(time, len_, num_frames, dt):
    """utils/motion_lib.py:263-272."""
    phase = time / len_
    raw = phase
    phase = torch.clip(phase, 0.0, 1.0)
    var = phase * (num_frames - 1)
    frame_idx0 = var.long()
    frame_idx1 = frame_idx0 + 1 if _MUT == 'i1_unclamped' else torch.min(frame_idx0 + 1, num_frames - 1)
    blend = (time - (frame_idx1 if _MUT == 'blend_from_i1' else frame_idx0) * dt) / dt
    return frame_idx0, frame_idx1, blend, raw, var


def local_rotation_to_dof(local_rot, body_ids, dof_offsets):
    """utils/motion_lib.py:296-324.  Decisions per joint: the angle-axis default; variables: sin_theta, w; and the acos
    allowance of every dof (module docstring)."""
    n = local_rot.shape[0]
    dof_pos = torch.zeros((n, dof_offsets[-1]), dtype=local_rot.dtype)
    allow = torch.zeros_like(dof_pos)
    masks, sins, ws, thetas = [], [], [], []
    for j in range(len(body_ids)):
        joint_offset = dof_offsets[j]
        joint_size = dof_offsets[j + 1] - joint_offset
        joint_q = local_rot[:, body_ids[j]]
        angle, axis, mask, sin_theta = quat_to_angle_axis(joint_q)
        per_angle = torch.where(mask, EPS23 / sin_theta.abs().clamp_min(1e-30), torch.zeros_like(sin_theta))
        if joint_size == 3:
            dof_pos[:, joint_offset:joint_offset + 3] = angle.unsqueeze(-1) * axis
            thetas.append(torch.zeros_like(angle))
            allow[:, joint_offset:joint_offset + 3] = per_angle.unsqueeze(-1) * axis.abs()
        elif joint_size == 1:
            theta = angle * axis[..., 2 if _MUT == 'hinge_z_dof' else 1]
            thetas.append(theta)
            if _MUT != 'hinge_no_second_wrap':
                theta = normalize_angle(theta)
            dof_pos[:, joint_offset] = theta
            allow[:, joint_offset] = per_angle * axis[..., 1].abs()
        else:
            raise AssertionError('Unsupported joint type')
        masks.append(mask); sins.append(sin_theta); ws.append(joint_q[:, 3])
    return dof_pos, {'aa_mask': torch.stack(masks, 1), 'aa_sin': torch.stack(sins, 1), 'aa_w': torch.stack(ws, 1),
                     'acos_allowance': allow, 'hinge_theta': torch.stack(thetas, 1)}


OUT_NAMES = ('root_pos', 'root_rot', 'dof_pos', 'root_vel', 'root_ang_vel', 'dof_vel', 'key_pos')
CLIP_FLOAT = ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'dt')


def get_motion_state(clips, motion_ids, motion_times, dtype):
    """utils/motion_lib.py:123-172 in ``dtype`` on the f32 clip tensors.  Returns (outputs dict, decisions dict)."""
    c = {k: clips[k].to(dtype) for k in CLIP_FLOAT}
    ids = motion_ids.long()
    t = motion_times.to(dtype)
    key_ids = torch.as_tensor(clips['key_body_ids'], dtype=torch.long)
    motion_len, num_frames, dt = c['lengths'][ids], clips['num_frames'].long()[ids], c['dt'][ids]
    i0, i1, blend, raw, var = calc_frame_blend(t, motion_len, num_frames, dt)
    starts = clips['length_starts'].long()[ids]
    f0l, f1l = i0 + starts, i1 + starts
    if _MUT == 'i1_unclamped':
        f1l = f1l.clamp_max(c['gts'].shape[0] - 1)
    root_pos0, root_pos1 = c['gts'][f0l, 0], c['gts'][f1l, 0]
    root_rot0, root_rot1 = c['grs'][f0l, 0], c['grs'][f1l, 0]
    local_rot0, local_rot1 = c['lrs'][f0l], c['lrs'][f1l]
    root_vel = c['grvs'][f1l if _MUT == 'root_vel_f1' else f0l]
    root_ang_vel = c['gravs'][f0l]
    key_pos0 = c['gts'][f0l.unsqueeze(-1), key_ids.unsqueeze(0)]
    key_pos1 = c['gts'][f1l.unsqueeze(-1), key_ids.unsqueeze(0)]
    dof_vel = c['dvs'][f0l]
    blend = blend.unsqueeze(-1)
    root_pos = (1.0 - blend) * root_pos0 + blend * root_pos1
    root_rot, d_root = slerp(root_rot0, root_rot1, blend)
    blend_exp = blend.unsqueeze(-1)
    key_pos = (1.0 - blend_exp) * key_pos0 + blend_exp * key_pos1
    local_rot, d_local = slerp(local_rot0, local_rot1, torch.unsqueeze(blend, axis=-1))
    dof_pos, d_dof = local_rotation_to_dof(local_rot, clips['dof_body_ids'], clips['dof_offsets'])
    out = dict(zip(OUT_NAMES, (root_pos, root_rot, dof_pos, root_vel, root_ang_vel, dof_vel, key_pos)))
    dec = {'f0': f0l, 'f1': f1l, 'phase_raw': raw, 'frame_var': var, 'root': d_root,
           'local': {k: v[:, clips['dof_body_ids']] for k, v in d_local.items()}}
    dec.update(d_dof)
    return out, dec


# ------------------------------------------------------------------------------------------------------------------------
# env/tasks/humanoid.py, env/tasks/humanoid_amp.py
# ------------------------------------------------------------------------------------------------------------------------
def dof_to_obs(pose, dof_offsets):
    """env/tasks/humanoid.py:523-552.  Decisions per joint: the exp-map default (True for a hinge) and its variable."""
    num_joints = len(dof_offsets) - 1
    dof_obs = torch.zeros(pose.shape[:-1] + (6 * num_joints,), dtype=pose.dtype)
    masks, variables, lens = [], [], []
    for j in range(num_joints):
        dof_offset = dof_offsets[j]
        dof_size = dof_offsets[j + 1] - dof_offsets[j]
        joint_pose = pose[:, dof_offset:(dof_offset + dof_size)]
        if dof_size == 3:
            joint_pose_q, mask, var = exp_map_to_quat(joint_pose)
            lens.append(torch.where(mask, 2.5 * EPS24 * torch.norm(joint_pose, dim=-1), torch.zeros_like(var)))
        elif dof_size == 1:
            axis = torch.tensor([0.0, 0.0, 1.0] if _MUT == 'hinge_z_obs' else [0.0, 1.0, 0.0], dtype=joint_pose.dtype)
            joint_pose_q = quat_from_angle_axis(joint_pose[..., 0], axis)
            mask, var = torch.ones(pose.shape[0], dtype=torch.bool), torch.ones(pose.shape[0], dtype=pose.dtype)
            lens.append(torch.zeros_like(var))
        else:
            raise AssertionError('Unsupported joint type')
        dof_obs[:, (j * 6):((j + 1) * 6)] = quat_to_tan_norm(joint_pose_q)
        masks.append(mask); variables.append(var)
    return dof_obs, {'em_mask': torch.stack(masks, 1), 'em_var': torch.stack(variables, 1), 'len_allowance': torch.stack(lens, 1)}


def build_amp_observations(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos, local_root_obs,
                           root_height_obs, dof_offsets):
    """env/tasks/humanoid_amp.py:280-316."""
    root_h = root_pos[:, 2:3]
    heading_rot, rot_dir = calc_heading_quat_inv(root_rot)
    if local_root_obs and _MUT != 'local_root_ignored':
        root_rot_obs = quat_mul(heading_rot, root_rot)
    else:
        root_rot_obs = root_rot
    root_rot_obs = quat_to_tan_norm(root_rot_obs)
    root_h_obs = root_h if root_height_obs else torch.zeros_like(root_h)
    local_root_vel = quat_rotate(heading_rot, root_vel)
    local_root_ang_vel = quat_rotate(heading_rot, root_ang_vel)
    local_key_body_pos = key_body_pos if _MUT == 'keys_not_relative' else key_body_pos - root_pos.unsqueeze(-2)
    n, K = local_key_body_pos.shape[0], local_key_body_pos.shape[1]
    heading_rot_expand = heading_rot.unsqueeze(-2).repeat((1, K, 1))
    local_end_pos = quat_rotate(heading_rot_expand.reshape(n * K, 4), local_key_body_pos.reshape(n * K, 3))
    flat_local_key_pos = local_end_pos.view(n, K * 3)
    dof_obs, dec = dof_to_obs(dof_pos, dof_offsets)
    dec['rot_dir'] = rot_dir
    obs = torch.cat((root_h_obs, root_rot_obs, local_root_vel, local_root_ang_vel, dof_obs, dof_vel, flat_local_key_pos), dim=-1)
    return obs, dec


def update_hist(hist, frame, shift):
    """env/tasks/humanoid_amp.py:248-266: slots move one step into the past, the new frame takes slot 0."""
    if shift:
        S = hist.shape[1]
        if _MUT == 'hist_towards_present':
            for i in range(S - 1):
                hist[:, i] = hist[:, i + 1]
        else:
            for i in reversed(range(S - 1)):
                hist[:, i + 1] = hist[:, i]
    hist[:, 0] = frame
    return hist


class RefBackend:
    """The f32 run of this module behind the two backend methods - with ``mutated()`` a wrong restatement as a 'device'."""

    def motion_state(self, clips, motion_ids, times):
        out, _ = get_motion_state(clips, motion_ids, times, torch.float32)
        return tuple(out[k] for k in OUT_NAMES)

    def build_amp_obs(self, root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos, dof_offsets,
                      local_root_obs, root_height_obs, hist, shift=True):
        frame, _ = build_amp_observations(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos,
                                          local_root_obs, root_height_obs, dof_offsets)
        update_hist(hist, frame, shift)


# ------------------------------------------------------------------------------------------------------------------------
# fixture builders: every input is constructed from its decision variable, nothing is drawn and rejected
# ------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dirs(g, n, d=3):
    v = torch.randn(n, d, generator=g, dtype=torch.float64)
    return v / v.norm(dim=-1, keepdim=True)


def _uniform(g, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)


def _qmul(a, b):                                          # plain Hamilton product (f64, fixture construction only)
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    return torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def quat_half_angle(axis, half):
    """Unit quaternion (f64) from a CHOSEN half angle about ``axis``."""
    half = torch.as_tensor(half, dtype=torch.float64)
    return torch.cat([axis * torch.sin(half).unsqueeze(-1), torch.cos(half).unsqueeze(-1)], -1)


def quat_near(E, k, g):
    """A quaternion whose dot product with the exactly-unit f32 quaternion E is 1 - k 2^-24: sin(half angle) = sqrt(k 2^-23)
    - 0.001 lies between k = 8 and k = 9.  The f32 dot product of the pair is off by at most 1.5 x 2^-24 (three additions),
    so k = 4 stays below and k = 12 above the threshold by more than the margin; the test asserts it."""
    d = torch.randn(4, generator=g, dtype=torch.float64)
    d = d - (d * E).sum() * E
    d = d / d.norm()
    c = 1.0 - k * EPS24
    return c * E + math.sqrt(1.0 - c * c) * d


H = torch.tensor([0.5, 0.5, 0.5, 0.5], dtype=torch.float64)              # exactly unit in f32: c == 1 with itself

# the character of the synthetic motion library: 3-dof joints and hinges, two bodies no joint uses, shuffled key bodies
LIB_OFFSETS = [0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 30, 33, 36, 37, 38, 39, 40, 41]
LIB_J = len(LIB_OFFSETS) - 1
LIB_BODIES = LIB_J + 3                                                     # root + joints + two unused
LIB_DOF_BODIES = [3, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 15, 17]  # joint j turns body LIB_DOF_BODIES[j]
LIB_KEYS = [17, 4, 19, 0, 9]
LIB_CLIPS = ((2, 1.0 / 30.0), (5, 1.0 / 60.0), (33, 1.0 / 32.0), (40, 1.0 / 30.0))   # (frames, dt)
# The rotation pattern of joint j in the 5-frame clip (clip 1); everything else is 'generic'.  sin_theta = sqrt(1 - w^2) of an
# f32 w is 0 (w = +-1), NaN (|w| > 1) or at least sqrt(2^-23) = 3.5e-4 (w one ulp below 1): 'identity' and 'w_above' are the
# side at or below 1e-5, every other pattern is above it by far more than the margin - nothing in between exists in f32.
SPECIAL = {0: 'generic', 1: 'antipodal', 2: 'exact_same', 3: 'exact_neg', 4: 'mid', 5: 'mid_flip', 6: 'just_generic',
           7: 'identity', 8: 'w_above', 9: 'w_neg', 10: 'generic', 11: 'generic', 12: 'generic', 13: 'antipodal',
           14: 'nonunit_hinge', 15: 'w_neg', 16: 'identity'}
ROOT_PATTERN = ('mid', 'antipodal', 'generic', 'root40')
PLANTED = ('exact_same', 'exact_neg', 'identity', 'w_above', 'nonunit_hinge', 'root40')   # decisions by exact arithmetic


def _pattern(name, nf, hinge, g):
    """[nf, 4] f64 quaternions of one body over a clip.  generic: a base rotation with w in [0.6, 0.85] turned by a half angle
    that alternates between 0 and 0.02 .. 0.04 (+- 0.004) - consecutive frames are 0.016 .. 0.044 apart (cos half theta <=
    1 - 1e-4), ten steps of extrapolation keep w in [0.15, 0.995]."""
    axis = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64) if hinge else _dirs(g, 1)[0]
    base = quat_half_angle(axis, float(_uniform(g, 1, math.acos(0.85), math.acos(0.6))))
    step = float(_uniform(g, 1, 0.02, 0.04))
    k = torch.arange(nf)
    half = step * (k % 2).double() + _uniform(g, nf, -0.002, 0.002)
    axis2 = axis if hinge else _dirs(g, 1)[0]
    q = _qmul(base.expand(nf, 4), quat_half_angle(axis2.expand(nf, 3), half))
    odd = (k % 2 == 1).unsqueeze(-1)
    if name == 'generic':
        return q
    if name == 'antipodal':
        return torch.where(odd, -q, q)
    if name == 'w_neg':
        return -q
    if name == 'exact_same':
        return H.expand(nf, 4).clone()
    if name == 'exact_neg':
        return torch.where(odd, -H, H).expand(nf, 4).clone()
    if name == 'identity':
        return torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(nf, 4).clone()
    if name == 'w_above':
        return torch.tensor([0.0, 0.0, 0.0, 1.0 + EPS23], dtype=torch.float64).expand(nf, 4).clone()
    if name == 'nonunit_hinge':                        # |axis_y| = 1.73: angle * axis_y passes -pi, the second wrap acts
        return torch.tensor([0.0, 1.5, 0.0, -0.5], dtype=torch.float64).expand(nf, 4).clone()
    if name in ('mid', 'mid_flip', 'just_generic'):
        near = quat_near(H, 12 if name == 'just_generic' else 4, g)
        return torch.where(odd, -near if name == 'mid_flip' else near, H).expand(nf, 4).clone()
    if name == 'root40':                               # (Ex, -near, Ex, Ex): flip + just generic twice, then c == 1
        ex = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
        near = -quat_near(ex, 12, g)
        return torch.stack([near if i % 4 == 1 else ex for i in range(nf)])
    raise KeyError(name)


def joint_pattern(clip, j):
    return SPECIAL[j] if clip == 1 else 'generic'


def motion_library(seed=5):
    """Four synthetic clips in one library (f32 tensors as ``DeviceMotionLib`` takes them; length_starts non-zero from clip 1)."""
    g = _gen(seed)
    B, D = LIB_BODIES, LIB_OFFSETS[-1]
    parts = {k: [] for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs')}
    for ci, (nf, dt) in enumerate(LIB_CLIPS):
        k = torch.arange(nf, dtype=torch.float64).view(nf, 1, 1)
        gts = torch.randn(1, B, 3, generator=g, dtype=torch.float64) + 0.05 * k * torch.randn(1, B, 3, generator=g, dtype=torch.float64) \
            + 0.01 * torch.randn(nf, B, 3, generator=g, dtype=torch.float64)
        lrs = torch.stack([_pattern('generic', nf, False, g) for _ in range(B)], 1)
        for j, b in enumerate(LIB_DOF_BODIES):
            hinge = LIB_OFFSETS[j + 1] - LIB_OFFSETS[j] == 1
            lrs[:, b] = _pattern(joint_pattern(ci, j), nf, hinge, g)
        grs = torch.stack([_pattern('generic', nf, False, g) for _ in range(B)], 1)
        grs[:, 0] = _pattern(ROOT_PATTERN[ci], nf, False, g)
        parts['gts'].append(gts); parts['grs'].append(grs); parts['lrs'].append(lrs)
        parts['grvs'].append(torch.randn(nf, 3, generator=g, dtype=torch.float64))
        parts['gravs'].append(torch.randn(nf, 3, generator=g, dtype=torch.float64))
        parts['dvs'].append(torch.randn(nf, D, generator=g, dtype=torch.float64))
    clips = {k: torch.cat(v).float() for k, v in parts.items()}
    nfs = torch.tensor([nf for nf, _ in LIB_CLIPS])
    clips['num_frames'] = nfs.to(torch.int32)
    clips['length_starts'] = (torch.cumsum(nfs, 0) - nfs).to(torch.int32)
    clips['dt'] = torch.tensor([dt for _, dt in LIB_CLIPS], dtype=torch.float64).float()
    clips['lengths'] = torch.tensor([dt * (nf - 1) for nf, dt in LIB_CLIPS], dtype=torch.float64).float()   # motion_lib.py:196
    clips.update(dof_body_ids=list(LIB_DOF_BODIES), dof_offsets=list(LIB_OFFSETS), key_body_ids=list(LIB_KEYS))
    return clips


TIME_KINDS = ('inside', 'below', 'beyond', 'inside', 'zero', 'length', 'inside', 'on_frame', 'history')
EXACT_KINDS = ('zero', 'length', 'on_frame')                                # the time sits on its threshold, exactly


def clip_times(clips, motion_ids, kinds, g):
    """Times from a CHOSEN frame and fraction: inside (k + f) dt with f in [0.05, 0.95]; below - u dt, u in [0.05, 3]; history
    down to - 10 dt; beyond length + u dt, u in [0.05, 3]; zero, length, on_frame (k / 32 on the 33-frame clip, whose
    products are exact; (k + 0.5) dt elsewhere) exactly."""
    out = []
    for m, kind in zip(motion_ids.tolist(), kinds):
        nf, dt = LIB_CLIPS[m]
        k = int(torch.randint(0, nf - 1, (1,), generator=g))
        f = float(_uniform(g, 1, 0.05, 0.95))
        u = float(_uniform(g, 1, 0.05, 3.0))
        if kind == 'inside':
            t = (k + f) * dt
        elif kind == 'below':
            t = -u * dt
        elif kind == 'history':
            t = -(u + 7.0) * dt
        elif kind == 'beyond':
            t = float(clips['lengths'][m]) + u * dt
        elif kind == 'zero':
            t = 0.0
        elif kind == 'length':
            t = float(clips['lengths'][m])
        else:
            t = k / 32.0 if m == 2 else (k + 0.5) * dt
        out.append(t)
    return torch.tensor(out, dtype=torch.float64).float()


MOTION_N = (1, 63, 64, 65, 130)


def motion_case(n, seed=0):
    g = _gen(1000 + 17 * n + seed)
    r = torch.arange(n)
    ids = ((r + (1 if n == 1 else 0)) % 4).to(torch.int32)
    kinds = [TIME_KINDS[(int(i) // 4 + int(i)) % len(TIME_KINDS)] for i in r]
    clips = motion_library()
    return {'name': f'n{n}', 'clips': clips, 'ids': ids, 'times': clip_times(clips, ids, kinds, g), 'kinds': kinds}


# ---- build_amp_obs ------------------------------------------------------------------------------------------------------
HUMANOID = [0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 28, 31]
LAYOUTS = {'humanoid': (HUMANOID, 6), 'hinge1': ([0, 1], 1), 'hinge32': (list(range(33)), 2), 'f255': (list(range(21)), 34),
           'k0': ([0, 3, 4], 0)}
TWO_PI = 2.0 * math.pi
# (name, length, single axis): single-axis maps have |e| = the f32 number itself in f32 and in f64
EXP_MENU = (('zero', 0.0, True), ('tiny', 1e-30, False), ('below', 0.9e-5, True), ('above', 1.1e-5, False),
            ('generic', 0.7, False), ('pi_minus', math.pi - 1e-3, False), ('pi_plus', math.pi + 1e-3, False),
            ('1.5pi', 1.5 * math.pi, False), ('2pi_minus', TWO_PI - 0.9e-5, True), ('2pi_plus', TWO_PI + 0.9e-5, True),
            ('seven', 7.0, False), ('generic', 2.1, False), ('huge', 1e30, True))
EXP_DEFAULT = ('zero', 'tiny', 'below', '2pi_minus', '2pi_plus', 'huge')
HINGE_MENU = (0.0, math.pi, -math.pi, 3.0, -3.0, 0.4, -1.7, 2.2)
VERTICAL = (0.5, -0.5, 0.5, 0.5)                   # its rotated x axis is exactly (0, 0, 1): heading = atan2(0, 0) = 0


def frame_size(layout):
    offs, K = LAYOUTS[layout]
    return 13 + 6 * (len(offs) - 1) + offs[-1] + 3 * K


def root_rotations(g, n):
    """Rz(yaw) Ry(pitch) Rx(roll) with |pitch| <= 1.45: the horizontal part of the rotated x axis is cos(pitch) >= 0.12."""
    e = lambda i: torch.eye(3, dtype=torch.float64)[i].expand(n, 3)
    qz = quat_half_angle(e(2), _uniform(g, n, -math.pi, math.pi) / 2)
    qy = quat_half_angle(e(1), _uniform(g, n, -1.45, 1.45) / 2)
    qx = quat_half_angle(e(0), _uniform(g, n, -math.pi, math.pi) / 2)
    return _qmul(qz, _qmul(qy, qx))


def obs_case(layout, N, S=2, shift=True, flags=(True, True), seed=0):
    offs, K = LAYOUTS[layout]
    J, D = len(offs) - 1, offs[-1]
    g = _gen(2000 + 31 * N + 7 * S + seed + sum(map(ord, layout)))
    root_rot = root_rotations(g, N)
    row_cls = torch.zeros(N, dtype=torch.long)
    if N >= 3:
        root_rot[2] = torch.tensor(VERTICAL, dtype=torch.float64)
        row_cls[2] = 1
    dof_pos = torch.zeros(N, D, dtype=torch.float64)
    joint_cls = torch.zeros(N, J, dtype=torch.long)                  # index into EXP_MENU; len(EXP_MENU) + i for hinge i
    for j in range(J):
        for r in range(N):
            if offs[j + 1] - offs[j] == 3:
                m = (r + 3 * j) % len(EXP_MENU)
                _, length, single = EXP_MENU[m]
                d = torch.eye(3, dtype=torch.float64)[(r + j) % 3] if single else _dirs(g, 1)[0]
                dof_pos[r, offs[j]:offs[j] + 3] = length * d
                joint_cls[r, j] = m
            else:
                m = (r + 3 * j) % len(HINGE_MENU)
                dof_pos[r, offs[j]] = HINGE_MENU[m]
                joint_cls[r, j] = len(EXP_MENU) + m
    f = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    root_pos = f(N, 3)
    inputs = {'root_pos': root_pos, 'root_rot': root_rot.float(), 'root_vel': f(N, 3), 'root_ang_vel': f(N, 3),
              'dof_pos': dof_pos.float(), 'dof_vel': f(N, D), 'key_body_pos': root_pos.unsqueeze(1) + f(N, K, 3)}
    return {'name': f'{layout}-N{N}-S{S}-shift{int(shift)}-{int(flags[0])}{int(flags[1])}', 'layout': layout, 'offs': offs, 'K': K,
            'N': N, 'S': S, 'shift': shift, 'flags': flags, 'inputs': inputs, 'row_cls': row_cls, 'joint_cls': joint_cls,
            'hist0': f(N, S, frame_size(layout))}


NONFINITE = (float('nan'), float('inf'), float('-inf'))
NONFINITE_WHERE = ('root_rot', 'hinge', 'exp_map', 'root_vel', 'key')


def nonfinite_case(flags=(True, True)):
    """One row per (operand, value) on the humanoid, three clean rows in front."""
    c = obs_case('humanoid', 3 + len(NONFINITE) * len(NONFINITE_WHERE), S=2, shift=False, flags=flags, seed=99)
    i = c['inputs']
    i['dof_pos'][i['dof_pos'].abs() > 1e20] = 0.5          # the 1e30 maps are held in the finite cases: only the plants here
    r = 3
    for where in NONFINITE_WHERE:
        for k, v in enumerate(NONFINITE):
            if where == 'root_rot':
                i['root_rot'][r, k] = v
            elif where == 'hinge':
                i['dof_pos'][r, 9] = v
            elif where == 'exp_map':
                i['dof_pos'][r, 3 + k] = v
                i['dof_pos'][r, 3 + (k + 1) % 3] = 0.3              # the other components finite and not zero
            elif where == 'root_vel':
                i['root_vel'][r, k] = v
            else:
                i['key_body_pos'][r, 2 + k, k] = v
            r += 1
    c['name'] = f'nonfinite-{int(flags[0])}{int(flags[1])}'
    c['nonfinite'] = True
    return c


def obs_plan():
    """Every case of ``build_amp_obs`` the two test files run."""
    plan = []
    for N in (1, 63, 64, 65, 130):
        plan.append(obs_case('humanoid', N, S=2, shift=True))
    for S in (1, 2, 10):
        for shift in (True, False):
            plan.append(obs_case('humanoid', 65, S=S, shift=shift, seed=1))
    for flags in ((True, True), (True, False), (False, True), (False, False)):
        plan.append(obs_case('humanoid', 70, S=3, shift=True, flags=flags, seed=2))
    # N F below / at / above a multiple of 256 (the shift kernel's last block): hinge1 has F = 23, hinge32 F = 243, f255 F = 255
    plan.append(obs_case('hinge1', 11, S=2))           # 253
    plan.append(obs_case('f255', 256, S=2))            # 255 x 256: full blocks only
    plan.append(obs_case('hinge1', 12, S=2))           # 276
    plan.append(obs_case('hinge1', 1, S=10))
    plan.append(obs_case('hinge32', 65, S=2))
    plan.append(obs_case('f255', 65, S=2))
    plan.append(obs_case('k0', 65, S=2))
    plan.append(obs_case('k0', 130, S=1, shift=False, flags=(False, False)))
    return plan


# ------------------------------------------------------------------------------------------------------------------------
# runs and comparisons
# ------------------------------------------------------------------------------------------------------------------------
GUARD = 96


def window(shape, dev, fill=float('nan'), dtype=torch.float32):
    """A contiguous tensor of ``shape`` inside a longer allocation filled with ``fill``; returns (view, whole)."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return whole[GUARD:GUARD + n].view(*shape), whole


def placed(t, dev):
    """``t`` inside a longer NaN-filled allocation on ``dev``."""
    v, _ = window(tuple(t.shape), dev)
    v.copy_(t)
    return v


def guards_intact(whole, n, what):
    g = torch.cat([whole[:GUARD], whole[GUARD + n:]]).cpu()
    COUNTS['sentinels'] += g.numel()
    assert bool(torch.isnan(g).all()), f'{what}: a guard word was written'


def _is_hip(be):
    return type(be).__name__ == 'HipBackend'


def run_motion_state(be, clips, ids, times, outs):
    """The entry with the caller's output tensors (the backend method allocates its own)."""
    if _is_hip(be):
        import ctypes as C
        from ase_amd import lib as L
        from ase_amd.backend import _ptr
        ia = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])
        L.check(be.lib.ase_hip_motion_state(
            _ptr(clips['gts']), _ptr(clips['grs']), _ptr(clips['lrs']), _ptr(clips['grvs']), _ptr(clips['gravs']), _ptr(clips['dvs']),
            clips['gts'].shape[1], _ptr(clips['lengths']), _ptr(clips['num_frames']), _ptr(clips['dt']), _ptr(clips['length_starts']),
            _ptr(ids), _ptr(times), ids.shape[0], ia(clips['dof_body_ids']), ia(clips['dof_offsets']), len(clips['dof_body_ids']),
            ia(clips['key_body_ids']), len(clips['key_body_ids']), *[_ptr(o) for o in outs], be._stream()), 'motion_state')
    else:
        for o, r in zip(outs, be.motion_state(clips, ids, times)):
            o.copy_(r)


def run_build(be, i, offs, flags, hist, shift):
    """``build_amp_obs``; without key bodies the device entry gets a NULL ``key_body_pos``."""
    if _is_hip(be) and i['key_body_pos'].shape[1] == 0:
        import ctypes as C
        from ase_amd import lib as L
        from ase_amd.backend import _ptr
        o = (C.c_int32 * len(offs))(*offs)
        L.check(be.lib.ase_hip_build_amp_obs(_ptr(i['root_pos']), _ptr(i['root_rot']), _ptr(i['root_vel']), _ptr(i['root_ang_vel']),
                                             _ptr(i['dof_pos']), _ptr(i['dof_vel']), None, hist.shape[0], offs[-1], 0, o,
                                             len(offs) - 1, int(flags[0]), int(flags[1]), _ptr(hist), hist.shape[1], int(shift),
                                             be._stream()), 'build_amp_obs')
    else:
        be.build_amp_obs(i['root_pos'], i['root_rot'], i['root_vel'], i['root_ang_vel'], i['dof_pos'], i['dof_vel'],
                         i['key_body_pos'], offs, flags[0], flags[1], hist, shift=shift)


def device_clips(clips, dev):
    d = {k: placed(clips[k], dev) for k in CLIP_FLOAT}
    d.update({k: clips[k].to(dev) for k in ('num_frames', 'length_starts')})
    d.update({k: clips[k] for k in ('dof_body_ids', 'dof_offsets', 'key_body_ids')})
    return d


def bitwise(got, want, what):
    got, want = got.cpu().contiguous(), want.cpu().float().contiguous()
    COUNTS['elements'] += got.numel()
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), f'{what}: not bitwise equal'


def within(key, got, r32, r64, labels=None, extra=None, names=None):
    """The module's bound, per decision class: ``labels`` (long, broadcastable to the values) splits the tensor into groups."""
    got = got.detach().cpu().double()
    assert got.shape == r64.shape, (key, got.shape, r64.shape)
    e_ref = (r32.double() - r64).abs()
    err = (got - r64).abs()
    labels = torch.zeros_like(r64, dtype=torch.long) if labels is None else labels.expand_as(r64)
    extra = torch.zeros_like(r64) if extra is None else extra.expand_as(r64)
    COUNTS['elements'] += got.numel()
    for lab in labels.unique().tolist():
        m = labels == lab
        gname = str(lab) if names is None else names[lab]
        allowed = 2 * float(e_ref[m].max()) + EPS23 * float(r64[m].abs().max()) + FLOOR + float(extra[m].max())
        worst = float(err[m].max())
        assert not torch.isnan(got[m]).any(), (key, gname, 'NaN')
        s = STATS.setdefault(key + (gname,), [0.0, 0.0, 0.0])
        s[0], s[1], s[2] = max(s[0], worst), max(s[1], float(e_ref[m].max())), max(s[2], worst / allowed)
        assert worst <= allowed, (key, gname, 'max |got - f64|', worst, 'allowed', allowed, 'elements', int(m.sum()))


def allowance_fraction(r32, r64, extra=None, level=1e-4):
    """Share of the elements whose own allowance 2 e_ref + 2^-23 |ref| + 1e-7 (+ acos term) is above ``level``."""
    a = 2 * (r32.double() - r64).abs() + EPS23 * r64.abs() + FLOOR + (0 if extra is None else extra)
    return float((a > level).double().mean())


def nonfinite_same(key, got, r32, r64):
    """Rows with NaN / inf: the expected value is the reference's (f32 run) - NaN where it has NaN, the same infinity, and
    the module's bound against f64 on the elements finite in both runs (against the f32 run where only f64 is not finite)."""
    got = got.detach().cpu()
    COUNTS['elements'] += got.numel()
    assert torch.equal(torch.isnan(got), torch.isnan(r32)), (key, 'NaN pattern', int((torch.isnan(got) != torch.isnan(r32)).sum()))
    inf = torch.isinf(r32)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], r32[inf]), (key, 'infinities')
    fin = torch.isfinite(r32)
    both = fin & torch.isfinite(r64)
    if both.any():
        within(key, got[both], r32[both], r64[both], names=['finite'])
    only = fin & ~both
    if only.any():
        within(key, got[only], r32[only], r32[only].double(), names=['finite_f32_only'])


# ---- motion_state -------------------------------------------------------------------------------------------------------
def motion_reference(case):
    if 'ref' not in case:
        o32, d32 = get_motion_state(case['clips'], case['ids'], case['times'], torch.float32)
        o64, d64 = get_motion_state(case['clips'], case['ids'], case['times'], torch.float64)
        case['ref'] = (o32, d32, o64, d64)
    return case['ref']


TIME_CLASS = {k: i for i, k in enumerate(sorted(set(TIME_KINDS)))}
TIME_NAMES = sorted(set(TIME_KINDS))
PATTERN_NAMES = sorted(set(SPECIAL.values()) | set(ROOT_PATTERN))


def motion_labels(case):
    """Per row: the time kind; per (row, dof): the joint's rotation pattern; per row: the root's."""
    ids = case['ids'].long()
    tk = torch.tensor([TIME_CLASS[k] for k in case['kinds']])
    J, D = LIB_J, LIB_OFFSETS[-1]
    jp = torch.tensor([[PATTERN_NAMES.index(joint_pattern(int(m), j)) for j in range(J)] for m in ids])
    dof_joint = torch.tensor([j for j in range(J) for _ in range(LIB_OFFSETS[j + 1] - LIB_OFFSETS[j])])
    rp = torch.tensor([PATTERN_NAMES.index(ROOT_PATTERN[int(m)]) for m in ids])
    return {'time': tk, 'joint': jp, 'dof': jp[:, dof_joint], 'root': rp}


def check_motion(be, dev, case):
    """One launch of ``motion_state`` on ``be`` against the f64 run."""
    o32, d32, o64, d64 = motion_reference(case)
    clips = device_clips(case['clips'], dev)
    ids, times = case['ids'].to(dev), placed(case['times'], dev)
    n = ids.shape[0]
    shapes = {k: tuple(o64[k].shape) for k in OUT_NAMES}
    wins = {k: window(shapes[k], dev) for k in OUT_NAMES}
    run_motion_state(be, clips, ids, times, [wins[k][0] for k in OUT_NAMES])
    for k in OUT_NAMES:
        guards_intact(wins[k][1], wins[k][0].numel(), f'motion_state {case["name"]} {k}')
    got = {k: wins[k][0].cpu() for k in OUT_NAMES}
    lab = motion_labels(case)
    for k in ('root_vel', 'root_ang_vel', 'dof_vel'):
        bitwise(got[k], o32[k], f'motion_state {case["name"]} {k}')
    key = lambda k: ('motion_state', k)
    within(key('root_pos'), got['root_pos'], o32['root_pos'], o64['root_pos'], lab['time'].view(n, 1), names=TIME_NAMES)
    within(key('key_pos'), got['key_pos'], o32['key_pos'], o64['key_pos'], lab['time'].view(n, 1, 1), names=TIME_NAMES)
    within(key('root_rot'), got['root_rot'], o32['root_rot'], o64['root_rot'], lab['root'].view(n, 1), names=PATTERN_NAMES)
    within(key('dof_pos'), got['dof_pos'], o32['dof_pos'], o64['dof_pos'], lab['dof'], extra=d64['acos_allowance'],
           names=PATTERN_NAMES)
    COUNTS['cases'] += 1
    return got


def check_chain(be, dev, case):
    """``motion_state`` -> ``build_amp_obs`` on the device outputs against the same chain in f64 (the demo fetch)."""
    clips = device_clips(case['clips'], dev)
    ids, times = case['ids'].to(dev), placed(case['times'], dev)
    o32, _, o64, _ = motion_reference(case)
    wins = [window(tuple(o64[k].shape), dev) for k in OUT_NAMES]
    outs = [w[0] for w in wins]
    run_motion_state(be, clips, ids, times, outs)
    for k, (v, whole_k) in zip(OUT_NAMES, wins):
        guards_intact(whole_k, v.numel(), 'chain motion_state ' + k)
    o = dict(zip(OUT_NAMES, outs))
    F = 13 + 6 * LIB_J + LIB_OFFSETS[-1] + 3 * len(LIB_KEYS)
    hist, whole = window((ids.shape[0], 1, F), dev)
    i = {'root_pos': o['root_pos'], 'root_rot': o['root_rot'], 'root_vel': o['root_vel'], 'root_ang_vel': o['root_ang_vel'],
         'dof_pos': o['dof_pos'], 'dof_vel': o['dof_vel'], 'key_body_pos': o['key_pos']}
    run_build(be, i, LIB_OFFSETS, (True, True), hist, False)
    guards_intact(whole, hist.numel(), 'chain')
    arg = lambda oo: (oo['root_pos'], oo['root_rot'], oo['root_vel'], oo['root_ang_vel'], oo['dof_pos'], oo['dof_vel'], oo['key_pos'])
    f32, _ = build_amp_observations(*arg(o32), True, True, LIB_OFFSETS)
    f64, _ = build_amp_observations(*arg(o64), True, True, LIB_OFFSETS)
    # per column block and decision class, as check_obs: rows by the kind of their time, joints by their rotation pattern
    got, lab = hist[:, 0].cpu(), motion_labels(case)
    n, J, D = ids.shape[0], LIB_J, LIB_OFFSETS[-1]
    od = 13 + 6 * J
    rows = lab['time'].view(n, 1)
    bitwise(got[:, od:od + D], o32['dof_vel'], 'chain dof_vel columns')
    within(('chain', 'height'), got[:, 0:1], f32[:, 0:1], f64[:, 0:1], rows, names=TIME_NAMES)
    within(('chain', 'root'), got[:, 1:13], f32[:, 1:13], f64[:, 1:13], rows, names=TIME_NAMES)
    within(('chain', 'keys'), got[:, od + D:], f32[:, od + D:], f64[:, od + D:], rows, names=TIME_NAMES)
    within(('chain', 'joints'), got[:, 13:od].reshape(n, J, 6), f32[:, 13:od].view(n, J, 6), f64[:, 13:od].view(n, J, 6),
           lab['joint'].view(n, J, 1), names=PATTERN_NAMES)
    COUNTS['cases'] += 1


# ---- build_amp_obs ------------------------------------------------------------------------------------------------------
def obs_reference(case):
    if 'ref' not in case:
        i = case['inputs']
        arg = lambda dt: [i[k].to(dt) for k in ('root_pos', 'root_rot', 'root_vel', 'root_ang_vel', 'dof_pos', 'dof_vel', 'key_body_pos')]
        f32, d32 = build_amp_observations(*arg(torch.float32), case['flags'][0], case['flags'][1], case['offs'])
        f64, d64 = build_amp_observations(*arg(torch.float64), case['flags'][0], case['flags'][1], case['offs'])
        case['ref'] = (f32, d32, f64, d64)
    return case['ref']


JOINT_NAMES = [m[0] for m in EXP_MENU] + [f'hinge{a:+.2f}' for a in HINGE_MENU]
HUGE = [m[0] for m in EXP_MENU].index('huge')


def check_obs(be, dev, case):
    """One launch of ``build_amp_obs`` on ``be``: the frame against the f64 run, copies, the history and the guards bitwise."""
    f32, d32, f64, d64 = obs_reference(case)
    N, S, offs, K = case['N'], case['S'], case['offs'], case['K']
    J, D = len(offs) - 1, offs[-1]
    F = f64.shape[1]
    i = {k: placed(v, dev) for k, v in case['inputs'].items()}
    hist, whole = window((N, S, F), dev)
    hist.copy_(case['hist0'])
    run_build(be, i, offs, case['flags'], hist, case['shift'])
    guards_intact(whole, hist.numel(), f'build_amp_obs {case["name"]}')
    got = hist.cpu()
    name = f'build_amp_obs {case["name"]}'
    if case['shift']:
        bitwise(got[:, 1:], case['hist0'][:, :-1], name + ' shifted slots')
    else:
        bitwise(got[:, 1:], case['hist0'][:, 1:], name + ' untouched slots')
    fr = got[:, 0]
    od = 13 + 6 * J
    bitwise(fr[:, 0], f32[:, 0], name + ' column 0')
    bitwise(fr[:, od:od + D], case['inputs']['dof_vel'], name + ' dof_vel columns')
    if case.get('nonfinite'):
        for blk, (a, b) in {'root': (1, 13), 'joints': (13, od), 'keys': (od + D, F)}.items():
            nonfinite_same(('build_amp_obs', blk + ' nonfinite'), fr[:, a:b], f32[:, a:b], f64[:, a:b])
        COUNTS['cases'] += 1
        return got
    key = lambda k: ('build_amp_obs', k)
    rows = case['row_cls'].view(N, 1)
    within(key('root'), fr[:, 1:13], f32[:, 1:13], f64[:, 1:13], rows, names=['generic', 'vertical'])
    if K:
        within(key('keys'), fr[:, od + D:], f32[:, od + D:], f64[:, od + D:], rows, names=['generic', 'vertical'])
    # the huge exponential map: its length overflows in f32 alone, so the f32 run is the expectation there
    jc = case['joint_cls'].view(N, J, 1)
    j64 = torch.where(jc == HUGE, f32[:, 13:od].view(N, J, 6).double(), f64[:, 13:od].view(N, J, 6))
    within(key('joints'), fr[:, 13:od].reshape(N, J, 6), f32[:, 13:od].view(N, J, 6), j64, jc,
           extra=d64['len_allowance'].double().view(N, J, 1), names=JOINT_NAMES)
    COUNTS['cases'] += 1
    return got


def report():
    return {'counts': dict(COUNTS), 'stats': {' | '.join(k): {'max_err': v[0], 'max_e_ref': v[1], 'err_over_allowed': v[2]}
                                              for k, v in sorted(STATS.items())}}
