"""CPU stand-in of ``HipBackend.env_pre_step`` / ``env_post_step`` with the same signatures, COMPOSED from the
stand-ins that are already pinned - ``EmuEnvTensors`` (observation, reset, task observation and reward) and
``EmuAmpReset.build_amp_obs`` (the AMP frame and the history shift) - so that it restates none of their arithmetic: what is new
here is the order, the progress increment, the recovery mask, the clip and the action / target expressions.  With the reset and
target-draw stand-ins mixed in, ``ase_amd.humanoid_env.HumanoidEnv`` runs on it.  TEST INFRASTRUCTURE ONLY."""
import torch

from ase_amd import lib as L
from tests.emu_env_tensors import EmuEnvTensors
from tests.emu_task_reset import EmuTaskReset
from tests.ref_amp_reset_due import EmuAmpResetDue


class EmuEnvStep(EmuEnvTensors, EmuTaskReset, EmuAmpResetDue):
    name = "emu-env-step"
    device = torch.device('cpu')

    def env_pre_step(self, actions_in, actions, targets, clip_actions=1.0, pd_offset=None, pd_scale=None, motor_efforts=None,
                     power_scale=1.0, root_states=None, prev_root_pos=None, recovery_counter=None):
        assert (pd_offset is None) == (pd_scale is None) and (pd_offset is None) != (motor_efforts is None)
        actions.copy_(torch.clamp(actions_in, -clip_actions, clip_actions))
        if pd_offset is not None:
            targets.copy_(pd_offset + pd_scale * actions)
        else:
            targets.copy_(actions * motor_efforts.unsqueeze(0) * power_scale)
        if prev_root_pos is not None:
            prev_root_pos.copy_(root_states[:, 0:3])
        if recovery_counter is not None:
            recovery_counter.sub_(1).clamp_min_(0)

    def env_post_step(self, body_pos, body_rot, body_vel, body_ang_vel, contact_forces, progress_buf, obs, reward, reset, terminated,
                      termination_heights, contact_body_ids, max_episode_length, enable_early_termination, local_root_obs,
                      root_height_obs, col_offset=0, clip_obs=float('inf'), task_kind=None, enable_task_obs=True, task_col_offset=None,
                      root_states=None, prev_root_pos=None, tar_a=None, tar_b=None, tar_speed=None, tar_states=None, reach_body_id=0,
                      dt=0.0, tar_contact_forces=None, strike_body_ids=None, recovery_counter=None, hist=None, dof_pos=None,
                      dof_vel=None, dof_offsets=None, key_body_ids=None):
        B = body_pos.shape[1]
        F = 15 * B - 2
        progress_buf += 1
        self.humanoid_obs_max(body_pos, body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs, obs, col_offset)
        cols = [(col_offset, F)]
        if task_kind is not None:
            if enable_task_obs:
                tc = col_offset + F if task_col_offset is None else task_col_offset
                self.task_obs(task_kind, obs, tc, None, root_states=root_states, tar_a=tar_a, tar_b=tar_b,
                              tar_speed=tar_speed if torch.is_tensor(tar_speed) else None, tar_states=tar_states)
                cols.append((tc, L.TASK_OBS_COLS[task_kind]))
            if task_kind == L.TASK_REACH:
                self.task_reward(task_kind, reward, tar_a=tar_a, body_pos=body_pos, body_id=reach_body_id)
            else:
                self.task_reward(task_kind, reward, root_states=root_states, prev_root_pos=prev_root_pos, tar_a=tar_a, tar_b=tar_b,
                                 tar_speed=tar_speed, tar_states=tar_states, dt=dt)
        else:
            reward.fill_(1.0)
        self.humanoid_reset(progress_buf, contact_forces, body_pos, termination_heights, contact_body_ids, max_episode_length,
                            enable_early_termination, reset, terminated, tar_contact_forces, strike_body_ids)
        if recovery_counter is not None:
            rec = recovery_counter > 0
            reset.masked_fill_(rec, 0)
            terminated.masked_fill_(rec, 0)
        if hist is not None:
            self.build_amp_obs(body_pos[:, 0], body_rot[:, 0], body_vel[:, 0], body_ang_vel[:, 0], dof_pos, dof_vel,
                               body_pos[:, list(key_body_ids)], dof_offsets, local_root_obs, root_height_obs, hist, shift=True)
        for c0, w in cols:
            obs[:, c0:c0 + w] = torch.clamp(obs[:, c0:c0 + w], -clip_obs, clip_obs)
