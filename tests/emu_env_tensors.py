"""Plain-torch restatement of the environment-side backend methods: ``humanoid_obs_max``, ``humanoid_reset``,
``task_obs``, ``task_reward`` with the signatures of ``ase_amd.backend.HipBackend``.  TEST INFRASTRUCTURE ONLY: the CPU stand-in
for ``ase_amd.env_tensors.HumanoidTensors`` in the host tests, and the torch leg of ``scripts/bench_extra.py --only env-tensors``
(it runs on whatever device its operands live on).

Written from the contract in include/ase_hip.h, following env/tasks/humanoid.py:592-636 (observation), :645-672 and
env/tasks/humanoid_strike.py:255-297 (reset), humanoid_heading.py:231-289, humanoid_location.py:169-232,
humanoid_reach.py:174-196, humanoid_strike.py:193-252 (task observations / rewards) under /root/reference/ase; the quaternion
algebra is oracle/amp_obs.py's (xyzw, Hamilton product)."""
import torch

from ase_amd import lib as L
from oracle import amp_obs as A


def _rows(obs, env_ids):
    return slice(None) if env_ids is None else env_ids.long()


def _rot3(hq, v):
    """quat_rotate of [n, k, 3] vectors by one quaternion per row."""
    n, k = v.shape[0], v.shape[1]
    return A.quat_rotate(hq.unsqueeze(1).expand(n, k, 4).reshape(-1, 4), v.reshape(-1, 3)).view(n, k, 3)


def _heading_quat(q):
    """utils/torch_utils.py:131-141: rotation about z by the heading of q."""
    ex = torch.zeros_like(q[:, :3]); ex[:, 0] = 1
    d = A.quat_rotate(q, ex)
    ez = torch.zeros_like(q[:, :3]); ez[:, 2] = 1
    return A.quat_from_angle_axis(torch.atan2(d[:, 1], d[:, 0]), ez)


def _pad3(xy):
    return torch.cat([xy, torch.zeros_like(xy[:, :1])], -1)


class EmuEnvTensors:
    name = "emu-env"
    device = torch.device('cpu')

    # Every comparison and clamp the reference branches on, one method each, so that tests/test_env_edges_emu.py can restate a
    # single term wrongly and show which recorded case notices.
    _loud = staticmethod(lambda force, threshold: force > threshold)               # |contact component| against 0.1 / 1.0
    _low = staticmethod(lambda height, threshold: height < threshold)
    _started = staticmethod(lambda progress: progress > 1)
    _timed_out = staticmethod(lambda progress, max_len: progress >= max_len - 1)
    _stopped = staticmethod(lambda speed: speed <= 0)
    _near = staticmethod(lambda pos_err: pos_err < 0.5)
    _upright = staticmethod(lambda rot_err: rot_err < 0.2)
    _clamp0 = staticmethod(lambda x: x.clamp_min(0.0))                             # torch.clamp_min: a NaN stays NaN
    _force_cols, _tar_cols = 3, 2                                                  # components of a force / of the target's that count
    _mask_height, _strike_falls = True, True

    # ---- humanoid.py:592-636
    def humanoid_obs_max(self, body_pos, body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs, obs, col_offset=0,
                         env_ids=None):
        r = _rows(obs, env_ids)
        pos, rot, vel, ang = body_pos[r], body_rot[r], body_vel[r], body_ang_vel[r]
        n, B = pos.shape[0], pos.shape[1]
        if n == 0:
            return
        root_pos, root_rot = pos[:, 0], rot[:, 0]
        hq = A.heading_quat_inv(root_rot)
        root_h = root_pos[:, 2:3] if root_height_obs else torch.zeros_like(root_pos[:, 2:3])
        local_pos = _rot3(hq, pos - root_pos.unsqueeze(1))[:, 1:].reshape(n, -1)          # the root's own position is dropped
        local_rot = A.quat_mul(hq.unsqueeze(1).expand(n, B, 4).reshape(-1, 4), rot.reshape(-1, 4))
        rot_obs = A.quat_to_tan_norm(local_rot).view(n, 6 * B).clone()
        if local_root_obs:                                                                 # the RAW root rotation (humanoid.py:620-622)
            rot_obs[:, 0:6] = A.quat_to_tan_norm(root_rot)
        out = torch.cat([root_h, local_pos, rot_obs, _rot3(hq, vel).reshape(n, -1), _rot3(hq, ang).reshape(n, -1)], -1)
        obs[r, col_offset:col_offset + out.shape[1]] = out

    # ---- humanoid.py:645-672, humanoid_strike.py:255-297
    def humanoid_reset(self, progress_buf, contact_forces, body_pos, termination_heights, contact_body_ids, max_episode_length,
                       enable_early_termination, reset, terminated, tar_contact_forces=None, strike_body_ids=None):
        assert (tar_contact_forces is None) == (strike_body_ids is None)
        B = body_pos.shape[1]
        term = torch.zeros_like(progress_buf)
        if enable_early_termination:
            keep = torch.ones(B, dtype=torch.bool, device=body_pos.device)
            keep[list(contact_body_ids)] = False
            # any component above the threshold, not the maximum above it: a NaN beside a loud component does not hide it
            force = contact_forces[..., :self._force_cols].abs()                           # [n, B, 3]
            other = keep.clone()
            if strike_body_ids is not None:
                other[list(strike_body_ids)] = False
            fall_contact = (self._loud(force, 0.1).any(-1) & (keep if self._strike_falls else other)).any(-1)
            low = self._low(body_pos[..., 2], termination_heights)
            fall_height = ((low & keep) if self._mask_height else low).any(-1)
            failed = fall_contact & fall_height
            if strike_body_ids is not None:
                tar_hit = self._loud(tar_contact_forces[:, 0:self._tar_cols].abs(), 1.0).any(-1)
                failed = failed | (tar_hit & (self._loud(force, 1.0).any(-1) & other).any(-1))
            term = (failed & self._started(progress_buf)).to(progress_buf.dtype)
        terminated.copy_(term)
        reset.copy_(torch.where(self._timed_out(progress_buf, max_episode_length), torch.ones_like(term), term))

    # ---- task observations
    def task_obs(self, kind, obs, col_offset=0, env_ids=None, root_states=None, tar_a=None, tar_b=None, tar_speed=None,
                 tar_states=None):
        r = _rows(obs, env_ids)
        rs = root_states[r]
        if rs.shape[0] == 0:
            return
        hq = A.heading_quat_inv(rs[:, 3:7])
        if kind == L.TASK_HEADING:
            assert tar_states is None
            out = torch.cat([A.quat_rotate(hq, _pad3(tar_a[r]))[:, :2], tar_speed[r].unsqueeze(-1),
                             A.quat_rotate(hq, _pad3(tar_b[r]))[:, :2]], -1)
        elif kind == L.TASK_LOCATION:
            assert tar_b is None and tar_speed is None and tar_states is None
            out = A.quat_rotate(hq, _pad3(tar_a[r]) - rs[:, 0:3])[:, :2]
        elif kind == L.TASK_REACH:
            assert tar_b is None and tar_speed is None and tar_states is None
            out = A.quat_rotate(hq, tar_a[r])
        else:
            assert tar_a is None and tar_b is None and tar_speed is None
            ts = tar_states[r]
            rel = ts[:, 0:3] - rs[:, 0:3]
            rel = torch.cat([rel[:, :2], ts[:, 2:3]], -1)                                   # the target's height stays absolute
            out = torch.cat([A.quat_rotate(hq, rel), A.quat_to_tan_norm(A.quat_mul(hq, ts[:, 3:7])),
                             A.quat_rotate(hq, ts[:, 7:10]), A.quat_rotate(hq, ts[:, 10:13])], -1)
        obs[r, col_offset:col_offset + out.shape[1]] = out

    # ---- task rewards (the constants are the reference's literals, lines in csrc/env_obs.hip)
    def _speed_reward(self, tar_dir, root_pos, prev_root_pos, tar_speed, dt):
        root_vel = (root_pos - prev_root_pos) / dt
        speed = (tar_dir * root_vel[:, :2]).sum(-1)
        err = self._clamp0(tar_speed - speed)
        r = torch.exp(-4.0 * (err * err))
        return torch.where(self._stopped(speed), torch.zeros_like(r), r)

    def task_reward(self, kind, reward, root_states=None, prev_root_pos=None, tar_a=None, tar_b=None, tar_speed=None,
                    tar_states=None, body_pos=None, body_id=0, dt=0.0):
        if kind == L.TASK_REACH:
            d = tar_a - body_pos[:, body_id]
            reward.copy_(torch.exp(-4.0 * (d * d).sum(-1)))
            return
        root_pos = root_states[:, 0:3]
        if kind == L.TASK_HEADING:
            root_vel = (root_pos - prev_root_pos) / dt
            speed = (tar_a * root_vel[:, :2]).sum(-1)
            tangent = (root_vel[:, :2] - speed.unsqueeze(-1) * tar_a).sum(-1)
            err = tar_speed - speed
            dir_r = torch.exp(-0.25 * (err * err + 0.1 * tangent * tangent))
            dir_r = torch.where(self._stopped(speed), torch.zeros_like(dir_r), dir_r)
            ex = torch.zeros_like(root_pos); ex[:, 0] = 1
            facing = A.quat_rotate(_heading_quat(root_states[:, 3:7]), ex)
            face_r = self._clamp0((tar_b * facing[:, :2]).sum(-1))
            reward.copy_(0.7 * dir_r + 0.3 * face_r)
        elif kind == L.TASK_LOCATION:
            diff = tar_a - root_pos[:, :2]
            pos_err = (diff * diff).sum(-1)
            tar_dir = torch.nn.functional.normalize(diff, dim=-1)
            vel_r = self._speed_reward(tar_dir, root_pos, prev_root_pos, float(tar_speed), dt)
            ex = torch.zeros_like(root_pos); ex[:, 0] = 1
            facing = A.quat_rotate(_heading_quat(root_states[:, 3:7]), ex)
            face_r = self._clamp0((tar_dir * facing[:, :2]).sum(-1))
            near = self._near(pos_err)
            one = torch.ones_like(vel_r)
            reward.copy_(0.5 * torch.exp(-0.5 * pos_err) + 0.4 * torch.where(near, one, vel_r) + 0.1 * torch.where(near, one, face_r))
        else:
            ez = torch.zeros_like(root_pos); ez[:, 2] = 1
            rot_err = A.quat_rotate(tar_states[:, 3:7], ez)[:, 2]
            tar_dir = torch.nn.functional.normalize(tar_states[:, 0:2] - root_pos[:, :2], dim=-1)
            vel_r = self._speed_reward(tar_dir, root_pos, prev_root_pos, 1.0, dt)
            r = 0.6 * self._clamp0(1.0 - rot_err) + 0.4 * vel_r
            reward.copy_(torch.where(self._upright(rot_err), torch.ones_like(r), r))


# ---- the fixture tests/golden/env_tensors.pt (scripts/make_golden_env.py) -------------------------------------------------
def golden_obs_max(G, tag, local_root_obs, root_height_obs):
    """The reference's humanoid observation for a flag combination: the file keeps the (True, True) matrix and, per combination,
    the seven columns that depend on the flags (asserted bitwise by the generator)."""
    out = G[tag]['obs_max'].clone()
    out[:, G['obs_max_flag_cols']] = G[tag]['obs_max_flag_cols'][(local_root_obs, root_height_obs)]
    return out


def golden_state(G, device='cpu'):
    """The fixture's inputs under the names HumanoidTensors reads, plus the per-task target tensors."""
    i = {k: v.to(device) for k, v in G['inputs'].items()}
    s = {'rigid_body_pos': i['body_pos'], 'rigid_body_rot': i['body_rot'], 'rigid_body_vel': i['body_vel'],
         'rigid_body_ang_vel': i['body_ang_vel'], 'humanoid_root_states': i['root_states'], 'contact_forces': i['contact_forces'],
         'prev_root_pos': i['prev_root_pos'], 'tar_dir': i['tar_dir'], 'tar_facing_dir': i['tar_face_dir'], 'tar_speed': i['tar_speed'],
         'target_states': i['tar_states'], 'tar_contact_forces': i['tar_contact_forces']}
    return i, s


def task_operands(G, i, task, what):
    """Keyword operands of task_obs / task_reward for a task of the fixture."""
    rs, prev = i['root_states'], i['prev_root_pos']
    if task == 'heading':
        kw = dict(root_states=rs, tar_a=i['tar_dir'], tar_b=i['tar_face_dir'], tar_speed=i['tar_speed'])
        return kw if what == 'obs' else dict(kw, prev_root_pos=prev, dt=G['dt'])
    if task == 'location':
        kw = dict(root_states=rs, tar_a=i['tar_pos_loc'])
        return kw if what == 'obs' else dict(kw, prev_root_pos=prev, tar_speed=G['tar_speed'], dt=G['dt'])
    if task == 'reach':
        if what == 'obs':
            return dict(root_states=rs, tar_a=i['tar_pos_reach'])
        return dict(tar_a=i['tar_pos_reach'], body_pos=i['body_pos'], body_id=G['reach_body_id'])
    kw = dict(root_states=rs, tar_states=i['tar_states'])
    return kw if what == 'obs' else dict(kw, prev_root_pos=prev, dt=G['dt'])


def allowance(G, name):
    """The float bar of the device tests: max |x - ref_f64| <= 2 e_ref + 1e-7, e_ref = what the reference's own f32 run loses
    against its f64 run (stored by the generator; the factor and the floor are reasoned in DESIGN §4)."""
    return 2.0 * G['e_ref'][name] + 1e-7
