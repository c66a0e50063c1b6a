"""Environment-side tensor functions on the device: what ``Humanoid`` / ``HumanoidAMPTask`` and the four
high-level tasks of the reference compute from the simulator's state tensors every step - ``_compute_observations``,
``_compute_reward``, ``_compute_reset`` (env/tasks/humanoid.py:385-413,592-672, humanoid_amp_task.py:51-64,
humanoid_heading.py / humanoid_location.py / humanoid_reach.py / humanoid_strike.py under /root/reference/ase) - as one
HIP launch per reference function (``csrc/env_obs.hip``); there is no host fallback.

``HumanoidTensors`` owns the buffers of the reference's task classes (``obs_buf``, ``rew_buf``, ``reset_buf``,
``terminate_buf``) and takes the simulator's tensors as a dict ``state`` under the reference's attribute names without the
underscore: ``rigid_body_pos / _rot / _vel / _ang_vel`` [n, B, 3 | 4], ``humanoid_root_states`` [n, 13],
``contact_forces`` [n, B, 3], ``prev_root_pos`` [n, 3], and per task ``tar_dir``, ``tar_facing_dir`` [n, 2] and
``tar_speed`` [n] (heading), ``tar_pos`` [n, 2] (location) or [n, 3] (reach), ``target_states`` [n, 13] and
``tar_contact_forces`` [n, 3] (strike).  Binding a simulator and drawing new targets stay with the caller; resetting the actors
is ``ase_amd.amp_env.HumanoidAMPTensors``.
"""
import torch

from . import lib as L

TASKS = {None: None, 'heading': L.TASK_HEADING, 'location': L.TASK_LOCATION, 'reach': L.TASK_REACH, 'strike': L.TASK_STRIKE}


def humanoid_obs_size(num_bodies):
    """Columns of compute_humanoid_observations_max: 1 + 3 (B - 1) + 6 B + 3 B + 3 B (253 for the 17-body humanoid)."""
    return 15 * int(num_bodies) - 2


class HumanoidTensors:
    def __init__(self, backend, num_envs, num_bodies, task=None, local_root_obs=True, root_height_obs=True,
                 contact_body_ids=(), termination_heights=0.15, max_episode_length=300, enable_early_termination=True,
                 strike_body_ids=None, dt=1.0 / 30.0, reach_body_id=None, tar_speed=1.0, device=None):
        if task not in TASKS:
            raise ValueError(f"task must be one of {list(TASKS)}, got {task!r}")
        if task == 'strike' and strike_body_ids is None:
            raise ValueError("the strike task needs strike_body_ids")
        if task == 'reach' and reach_body_id is None:
            raise ValueError("the reach task needs reach_body_id")
        self.be, self.task, self.kind = backend, task, TASKS[task]
        self.num_envs, self.num_bodies = int(num_envs), int(num_bodies)
        self.local_root_obs, self.root_height_obs = bool(local_root_obs), bool(root_height_obs)
        self.contact_body_ids = [int(b) for b in contact_body_ids]
        self.strike_body_ids = None if strike_body_ids is None else [int(b) for b in strike_body_ids]
        self.reach_body_id = reach_body_id
        self.max_episode_length, self.enable_early_termination = float(max_episode_length), bool(enable_early_termination)
        self.dt, self.tar_speed = float(dt), float(tar_speed)
        dev = torch.device(device if device is not None else getattr(backend, 'device', 'cpu'))
        self.device = dev
        h = torch.as_tensor(termination_heights, dtype=torch.float32)
        self.termination_heights = (h.expand(self.num_bodies) if h.dim() == 0 else h).contiguous().to(dev)
        if self.termination_heights.numel() != self.num_bodies:
            raise ValueError("termination_heights: one height or one per body")
        n = self.num_envs
        self.obs_buf = torch.zeros(n, self.get_obs_size(), dtype=torch.float32, device=dev)
        self.rew_buf = torch.zeros(n, dtype=torch.float32, device=dev)
        self.reset_buf = torch.ones(n, dtype=torch.int64, device=dev)      # all due for a reset at the start (base_task.py:52)
        self.terminate_buf = torch.zeros(n, dtype=torch.int64, device=dev)

    # ---- sizes (humanoid.py:107-108, humanoid_amp_task.py:18-26)
    def get_humanoid_obs_size(self):
        return humanoid_obs_size(self.num_bodies)

    def get_task_obs_size(self):
        return 0 if self.kind is None else L.TASK_OBS_COLS[self.kind]

    def get_obs_size(self):
        return self.get_humanoid_obs_size() + self.get_task_obs_size()

    # ---- per-step functions
    def _task_operands(self, state):
        s = state
        if self.task == 'heading':
            return dict(root_states=s['humanoid_root_states'], tar_a=s['tar_dir'], tar_b=s['tar_facing_dir'], tar_speed=s['tar_speed'])
        if self.task == 'strike':
            return dict(root_states=s['humanoid_root_states'], tar_states=s['target_states'])
        return dict(root_states=s['humanoid_root_states'], tar_a=s['tar_pos'])

    def compute_observations(self, state, env_ids=None):
        """``_compute_observations`` (humanoid_amp_task.py:51-64): humanoid and task columns side by side in obs_buf; with
        env_ids only those rows are recomputed (``obs_buf[env_ids] = obs``)."""
        if env_ids is not None:
            env_ids = torch.as_tensor(env_ids, device=self.device).to(torch.int32).contiguous()
        self.be.humanoid_obs_max(state['rigid_body_pos'], state['rigid_body_rot'], state['rigid_body_vel'], state['rigid_body_ang_vel'],
                                 self.local_root_obs, self.root_height_obs, self.obs_buf, 0, env_ids)
        if self.kind is not None:
            self.be.task_obs(self.kind, self.obs_buf, self.get_humanoid_obs_size(), env_ids, **self._task_operands(state))
        return self.obs_buf

    def compute_reward(self, state):
        """``_compute_reward`` of the task; without a task the reference's constant 1 (compute_humanoid_reward, humanoid.py:638-643)."""
        s = state
        if self.kind is None:
            self.rew_buf.fill_(1.0)
        elif self.task == 'heading':
            self.be.task_reward(self.kind, self.rew_buf, root_states=s['humanoid_root_states'], prev_root_pos=s['prev_root_pos'],
                                tar_a=s['tar_dir'], tar_b=s['tar_facing_dir'], tar_speed=s['tar_speed'], dt=self.dt)
        elif self.task == 'location':
            self.be.task_reward(self.kind, self.rew_buf, root_states=s['humanoid_root_states'], prev_root_pos=s['prev_root_pos'],
                                tar_a=s['tar_pos'], tar_speed=self.tar_speed, dt=self.dt)
        elif self.task == 'reach':
            self.be.task_reward(self.kind, self.rew_buf, tar_a=s['tar_pos'], body_pos=s['rigid_body_pos'], body_id=self.reach_body_id)
        else:
            self.be.task_reward(self.kind, self.rew_buf, root_states=s['humanoid_root_states'], prev_root_pos=s['prev_root_pos'],
                                tar_states=s['target_states'], dt=self.dt)
        return self.rew_buf

    def compute_reset(self, state, progress_buf):
        """``_compute_reset`` (humanoid.py:368-373; the strike task passes the target's contact forces too)."""
        strike = self.task == 'strike'
        self.be.humanoid_reset(progress_buf, state['contact_forces'], state['rigid_body_pos'], self.termination_heights,
                               self.contact_body_ids, self.max_episode_length, self.enable_early_termination, self.reset_buf,
                               self.terminate_buf, state['tar_contact_forces'] if strike else None,
                               self.strike_body_ids if strike else None)
        return self.reset_buf, self.terminate_buf


def compute_humanoid_obs_reduced(backend, root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos, dof_offsets,
                                 local_root_obs=True, root_height_obs=True):
    """``compute_humanoid_observations`` (env/tasks/humanoid.py:553-589), the non-max form: the same arithmetic as one frame of
    the AMP observation, so it is the existing builder with a history of one slot and no shift."""
    n = root_pos.shape[0]
    F = 13 + 6 * (len(dof_offsets) - 1) + dof_pos.shape[1] + 3 * key_body_pos.shape[1]
    obs = torch.zeros(n, 1, F, dtype=torch.float32, device=root_pos.device)
    backend.build_amp_obs(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos, dof_offsets, local_root_obs,
                          root_height_obs, obs, shift=False)
    return obs.view(n, F)
