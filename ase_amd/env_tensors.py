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
``tar_contact_forces`` [n, 3] (strike).

The targets are drawn and reset here as well (``csrc/task_reset.hip``): ``_reset_task`` of the heading, location
and reach tasks, ``HumanoidStrike._reset_target`` and the per-step ``_update_task`` (humanoid_heading.py:147-174,
humanoid_location.py:107-125, humanoid_reach.py:111-130, humanoid_strike.py:108-128) write the target tensors of ``state`` in
place, one launch each.  ``HumanoidTensors`` owns the change steps and a Philox stream position for the draws made on the
device; as in ``amp_env`` a reset is also available as a draw (``draw_task_reset`` -> a plan of device tensors, drawn with
torch under ``generator`` in the reference's call order) and an apply (``apply_task_reset``: the launch on those draws).
``update_task`` tests ``progress_buf >= change_steps`` inside the kernel: no ``nonzero``, no host synchronisation, recordable
in a launch program.  Binding a simulator and the viewer's marker updates (``_update_marker``) stay with the caller; resetting
the actors is ``ase_amd.amp_env.HumanoidAMPTensors``.
"""
import torch

from . import lib as L

# the reset parameters of a task where the caller gives none: ase/data/cfg/humanoid_sword_shield_heading / _location /
# _reach.yaml of the reference; the strike task's are literals of its constructor (humanoid_strike.py:19-22)
TASK_RESET_DEFAULTS = {
    'heading': dict(tar_speed_min=1.5, tar_speed_max=1.6, heading_change_steps_min=100, heading_change_steps_max=200,
                    enable_rand_heading=True),
    'location': dict(tar_change_steps_min=100, tar_change_steps_max=200, tar_dist_max=10.0),
    'reach': dict(tar_change_steps_min=50, tar_change_steps_max=100, tar_dist_max=1.0, tar_height_min=0.2, tar_height_max=2.0),
    'strike': dict(tar_dist_min=0.5, tar_dist_max=10.0, near_dist=1.5, near_prob=0.5),
}

TASKS = {None: None, 'heading': L.TASK_HEADING, 'location': L.TASK_LOCATION, 'reach': L.TASK_REACH, 'strike': L.TASK_STRIKE}


def humanoid_obs_size(num_bodies):
    """Columns of compute_humanoid_observations_max: 1 + 3 (B - 1) + 6 B + 3 B + 3 B (253 for the 17-body humanoid)."""
    return 15 * int(num_bodies) - 2


class HumanoidTensors:
    def __init__(self, backend, num_envs, num_bodies, task=None, local_root_obs=True, root_height_obs=True,
                 contact_body_ids=(), termination_heights=0.15, max_episode_length=300, enable_early_termination=True,
                 strike_body_ids=None, dt=1.0 / 30.0, reach_body_id=None, tar_speed=1.0, device=None, generator=None, seed=0,
                 tar_speed_min=None, tar_speed_max=None, heading_change_steps_min=None, heading_change_steps_max=None,
                 enable_rand_heading=None, tar_change_steps_min=None, tar_change_steps_max=None, tar_dist_min=None, tar_dist_max=None,
                 tar_height_min=None, tar_height_max=None, near_dist=None, near_prob=None):
        """The last thirteen are the task's reset parameters under the reference's attribute names - heading: tar_speed_min / _max,
        heading_change_steps_min / _max, enable_rand_heading; location / reach: tar_change_steps_min / _max, tar_dist_max (and
        tar_height_min / _max for reach); strike: tar_dist_min / _max, near_dist, near_prob.  None: the task's value in
        TASK_RESET_DEFAULTS; a parameter the task does not have is refused.
        generator: the torch generator of draw_task_reset; seed: the seed of the device-side draws (rng_state)."""
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
        p = dict(TASK_RESET_DEFAULTS.get(task, {}))
        given = dict(tar_speed_min=tar_speed_min, tar_speed_max=tar_speed_max, heading_change_steps_min=heading_change_steps_min,
                     heading_change_steps_max=heading_change_steps_max, enable_rand_heading=enable_rand_heading,
                     tar_change_steps_min=tar_change_steps_min, tar_change_steps_max=tar_change_steps_max, tar_dist_min=tar_dist_min,
                     tar_dist_max=tar_dist_max, tar_height_min=tar_height_min, tar_height_max=tar_height_max, near_dist=near_dist,
                     near_prob=near_prob)
        task_reset_params = {k: v for k, v in given.items() if v is not None}
        unknown = set(task_reset_params) - set(p)
        if unknown:
            raise ValueError(f"task {task!r} has no reset parameter {sorted(unknown)} (it has {sorted(p)})")
        p.update(task_reset_params)
        self.gen = generator
        self._steps_range = None                 # [low, high) of the change steps; the strike task has none
        for prefix in ('heading', 'tar'):
            if prefix + '_change_steps_min' in p:
                self._steps_range = (int(p.pop(prefix + '_change_steps_min')), int(p.pop(prefix + '_change_steps_max')))
                if self._steps_range[1] <= self._steps_range[0]:
                    raise ValueError(f"change steps are drawn from [min, max): {self._steps_range}")
        self._reset_params = p
        # all zero: every environment is due at its first update_task (humanoid_heading.py:30)
        self.change_steps = None if self._steps_range is None else torch.zeros(n, dtype=torch.int64, device=dev)
        self.rng_state = torch.tensor([int(seed), 0], dtype=torch.int64, device=dev)       # Philox {seed, offset} of the device draws

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

    # ---- targets: _reset_task / _reset_target / _update_task
    def _reset_operands(self, state, progress_buf):
        s = state
        kw = dict(self._reset_params)
        if self._steps_range is not None:
            kw.update(progress_buf=progress_buf, change_steps=self.change_steps, steps_low=self._steps_range[0],
                      steps_high=self._steps_range[1])
        if self.task == 'heading':
            kw.update(tar_a=s['tar_dir'], tar_b=s['tar_facing_dir'], tar_speed=s['tar_speed'])
        elif self.task == 'location':
            kw.update(root_states=s['humanoid_root_states'], tar_a=s['tar_pos'])
        elif self.task == 'reach':
            kw.update(tar_a=s['tar_pos'])
        else:
            kw.update(root_states=s['humanoid_root_states'], tar_states=s['target_states'])
        return kw

    def _ids(self, env_ids):
        return torch.as_tensor(env_ids, device=self.device).to(torch.int32).contiguous().view(-1)

    def draw_task_reset(self, env_ids):
        """The random part of ``_reset_task`` / ``_reset_target``, drawn with torch under ``generator`` in the reference's call
        order and shapes (so the same CPU seed gives the reference's draws) -> plan, a dict of device tensors: ``env_ids``
        int32 [n], ``u`` f32 [n, 3 | 2 | 3 | 4] and ``steps`` int64 [n] (None for strike).  None without a task."""
        if self.kind is None:
            return None
        ids = self._ids(env_ids)
        n, dev = ids.numel(), self.device
        rand = lambda *shape: torch.rand(*shape, device=dev, generator=self.gen)
        if self.task == 'heading':
            # without enable_rand_heading the reference takes zeros and draws nothing for the two angles
            angles = [rand(n), rand(n)] if self._reset_params['enable_rand_heading'] else [torch.zeros(n, device=dev)] * 2
            u = torch.stack(angles + [rand(n)], dim=-1)
        elif self.task == 'strike':
            u = torch.stack([rand([n]) for _ in range(4)], dim=-1)
        else:
            u = rand([n, L.TASK_RESET_DRAWS[self.kind]])
        steps = None
        if self._steps_range is not None:
            steps = torch.randint(low=self._steps_range[0], high=self._steps_range[1], size=(n,), device=dev, dtype=torch.int64,
                                  generator=self.gen)
        return {'env_ids': ids, 'u': u.contiguous(), 'steps': steps}

    def apply_task_reset(self, state, plan, progress_buf=None):
        """``_reset_task(env_ids)`` / ``_reset_target(env_ids)`` on the draws of a plan: one launch.  The plan's tensors are
        read when the launch runs.  The strike target is placed relative to the root the launch finds: call it after the
        actor reset (``HumanoidAMPTensors.apply_reset``), as the reference does (humanoid_strike.py:103-106)."""
        if self.kind is None:
            return
        self.be.task_reset(self.kind, env_ids=plan['env_ids'], u=plan['u'], steps=plan['steps'],
                           **self._reset_operands(state, progress_buf))

    def reset_task(self, state, env_ids, progress_buf=None):
        """``_reset_task(env_ids)`` / ``_reset_target(env_ids)`` with draws made on the device: one launch, the draws of
        environment e depend on (seed, stream position, e) only.  For strike as apply_task_reset: after the actor reset."""
        if self.kind is None:
            return
        self.be.task_reset(self.kind, env_ids=self._ids(env_ids), rng_state=self.rng_state, **self._reset_operands(state, progress_buf))

    def update_task(self, state, progress_buf):
        """``_update_task``, the per-step call: every environment with ``progress_buf >= change_steps`` gets a new target and
        new change steps; the test runs inside the launch (no nonzero, no host synchronisation).  Nothing for strike."""
        if self._steps_range is None:
            return
        self.be.task_reset(self.kind, rng_state=self.rng_state, **self._reset_operands(state, progress_buf))


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
