"""The view-motion task on the device: the reference's ``HumanoidViewMotion`` (env/tasks/humanoid_view_motion.py)
on the physics protocol of ``humanoid_env.HumanoidEnv`` - a HumanoidAMP that plays the motion library's clips through the
environment instead of simulating: every step the pose of each environment's clip at ``progress_buf * motion_dt`` is written
into the simulator's root and dof tensors with zero velocities and pushed.  It is what one looks at - observations, AMP frames -
before a clip that was just retargeted goes into a training run.

``ViewMotionEnv`` subclasses ``HumanoidEnv`` and leaves its code paths alone.  One step is::

    pre_physics_step     the clamped actions are copied; the forces applied are zeros (pdControl is forced off)
    physics.apply(zeros, False); physics.step()
    env_post_step        (one launch) the AMP class's post_physics_step: progress, observation, reward, AMP history.  Early
                         termination is off, and whatever its reset test writes is overwritten by the next launch
    motion_sync SYNC     (one launch, ``ase_hip_motion_sync``) reset_buf = progress_buf * motion_dt > clip length (strict),
                         terminate_buf = 0, the sampled pose into the root row and the dof state in place, velocities zero
    physics.push_state(all ids)

``reset`` / ``reset_done`` run the RESET launch - ``_reset_env_tensors``: the rows move on to clip ``(id + num_envs) mod
num_motions`` and their three buffers are cleared - then rebuild slot 0 of the AMP history and the observation of those rows
from the state as it is.  RESET writes no state: the reference's override does not call the base class's indexed set, so a
reset environment keeps showing the old clip's last pose until the next SYNC.  That is restated, not repaired.

``fused=False`` makes the same step from ``backend.motion_state`` and torch glue: the composition the launch is tested
against, bit for bit, made only of entries that existed before ``ase_hip_motion_sync``.

``motion_dt = controlFrequencyInv * sim dt``: the reference forces controlFrequencyInv to 1 for the simulator, so the physics'
``dt`` IS the simulator's step; ``controlFrequencyInv`` (default 1) is the one simulator key this class reads from env_cfg.

``ClipPhysics`` is a kinematic stand-in for the protocol: it owns packed state tensors in the simulator's layout and the SYNC
launch writes every rigid body straight into them, through the entry's optional outputs.  The bodies are the clip's OWN arrays -
``gts`` and ``grs``, every body's global translation and rotation, which the loader pins to poselib - blended by the reference's
two expressions: linear, as the sampler blends key-body positions, and ``slerp``, as it blends the root rotation.  It is not
forward kinematics from the dofs and not dynamics.  Body velocities are zero because view-motion zeroes the root's and the
dofs'.  As with a real simulator the bodies that step k + 1 observes are the pose synced at step k, one frame late."""
import torch

from . import lib as L
from .humanoid_env import BODY_KEYS, HumanoidEnv


class ViewMotionEnv(HumanoidEnv):
    def __init__(self, backend, physics, env_cfg, motion_lib, fused=True, seed=0, clip_observations=5.0, clip_actions=1.0):
        """env_cfg: the ``env`` section of the task yaml, plus ``controlFrequencyInv``.  pdControl is forced off and early
        termination with it (SYNC owns reset_buf / terminate_buf)."""
        if motion_lib is None:
            raise ValueError("the view-motion task plays a motion library: it needs a motion_lib")
        cfg = dict(env_cfg)
        self.motion_dt = int(cfg.pop('controlFrequencyInv', 1)) * float(physics.dt)
        cfg['pdControl'] = False
        cfg['enableEarlyTermination'] = False
        super().__init__(backend, physics, cfg, motion_lib=motion_lib, fused_step=fused, seed=seed,
                         clip_observations=clip_observations, clip_actions=clip_actions)
        self.fused = bool(fused)
        self._motion_lib = motion_lib
        n, dev = self.num_envs, self.device
        self.num_motions = int(motion_lib.num_motions())
        self.motion_ids = (torch.arange(n, dtype=torch.int64) % self.num_motions).to(torch.int32).to(dev)
        self._all_ids = torch.arange(n, dtype=torch.int32, device=dev)
        self.reset_ids = torch.full((n,), -1, dtype=torch.int32, device=dev)     # RESET's export: e where e was reset, else -1
        # a kinematic physics receives the rigid bodies from the launch; a simulator computes its own
        self._write_bodies = bool(getattr(physics, 'kinematic', False))
        B = int(physics.num_bodies)
        if self._write_bodies and motion_lib.clips['gts'].shape[1] != B:
            raise ValueError("the clips' skeleton is not the physics'")
        self._all_bodies = dict(motion_lib.clips, key_body_ids=list(range(B)))

    # ---- one step
    def pre_physics_step(self, actions):
        torch.clamp(actions, -self.clip_actions, self.clip_actions, out=self.actions)
        # self.targets stays zero: the forces of the reference's pre_physics_step

    def _body_outputs(self):
        s = self.physics.state
        return {k.replace('rigid_', ''): s[k] for k in BODY_KEYS} if self._write_bodies else {}

    def motion_sync(self):
        """_compute_reset + _motion_sync on the counters as they are."""
        s, clips = self.physics.state, self._motion_lib.clips
        root, dof_pos, dof_vel = s['humanoid_root_states'], s['dof_pos'], s['dof_vel']
        if self.fused:
            self.be.motion_sync(clips, self.motion_ids, self.progress_buf, self.reset_buf, self.terminate_buf, L.MOTION_SYNC,
                                self.motion_dt, root, dof_pos, dof_vel, **self._body_outputs())
            return
        ids = self.motion_ids
        t = self.progress_buf * self.motion_dt               # f32: the counter and the Python float both rounded to it
        self.reset_buf.copy_(t > clips['lengths'][ids.long()])
        self.terminate_buf.zero_()
        out = self.be.motion_state(self._all_bodies if self._write_bodies else clips, ids, t)
        root[:, 0:3], root[:, 3:7], root[:, 7:13] = out[0], out[1], 0.0
        dof_pos.copy_(out[2])
        dof_vel.zero_()
        if self._write_bodies:
            s['rigid_body_pos'].copy_(out[6])
            s['rigid_body_vel'].zero_()
            s['rigid_body_ang_vel'].zero_()
            rot = s['rigid_body_rot']
            rot[:, 0] = out[1]
            for b in range(1, rot.shape[1]):                 # the root rotation's expression on body b's rows of grs
                shifted = dict(clips, grs=clips['grs'][:, b:], key_body_ids=[0])
                rot[:, b] = self.be.motion_state(shifted, ids, t)[1]

    def post_physics_step(self):
        obs = super().post_physics_step()
        self.motion_sync()
        self.physics.push_state(self._all_ids)
        return obs

    def step(self, actions):
        self.pre_physics_step(actions)
        self.physics.apply(self.targets, False)
        self.physics.step()
        obs = self.post_physics_step()
        infos = {'terminate': self.terminate_buf, 'amp_obs': self.amp.amp_obs_buf.view(self.num_envs, self.amp.get_num_amp_obs())}
        return obs, self.rew_buf, self.reset_buf, infos

    # ---- resets: _reset_env_tensors, then _compute_observations(env_ids) and _init_amp_obs(env_ids) - with no actor reset the
    # latter is the current frame into slot 0 of those rows, nothing else
    def _advance(self, env_ids):
        if self.fused:
            self.be.motion_sync(self._motion_lib.clips, self.motion_ids, self.progress_buf, self.reset_buf, self.terminate_buf,
                                L.MOTION_RESET, env_ids=env_ids, ids_out=self.reset_ids if env_ids is None else None)
            return self.reset_ids if env_ids is None else env_ids
        n = self.num_envs
        if env_ids is None:
            due = self.reset_buf != 0
        else:
            ids = env_ids.long()
            due = torch.zeros(n, dtype=torch.bool, device=self.device)
            due[ids[(ids >= 0) & (ids < n)]] = True
        due &= (self.motion_ids >= 0) & (self.motion_ids < self.num_motions)
        self.motion_ids.copy_(torch.where(due, torch.remainder(self.motion_ids + n, self.num_motions), self.motion_ids))
        for buf in (self.progress_buf, self.reset_buf, self.terminate_buf):
            buf.masked_fill_(due, 0)
        if env_ids is None:
            self.reset_ids.copy_(torch.where(due, self._all_ids, -1))
            return self.reset_ids
        return env_ids

    def _after_reset(self, ids):
        s, packed = self._contiguous_state()
        self._compute_observations(s, ids)
        self.amp.compute_amp_observations(s, ids)
        return self._clipped_obs()

    def reset(self, env_ids=None):
        ids = self._all_ids if env_ids is None else torch.as_tensor(env_ids, device=self.device).view(-1).to(torch.int32).contiguous()
        if ids.numel() == 0:
            return self._clipped_obs()
        return self._after_reset(self._advance(ids))

    def reset_done(self, mask=None):
        """The device path: the rows with reset_buf != 0, decided inside the launch.  The host learns nothing."""
        return self._after_reset(self._advance(None))


class ClipPhysics:
    """The kinematic stand-in for the physics protocol (module docstring): packed state tensors in the simulator's layout -
    root tensor [n, 1 + K, 13] (the humanoid and K other actors, untouched), dof state [n, D, 2], rigid-body state [n, B, 13],
    contact forces [n, B, 3] = 0 - whose windows are ``state``.  ``apply`` ignores its targets, ``step`` and ``push_state`` do
    nothing: ``ViewMotionEnv``'s SYNC launch writes root, dofs and every body into the tensors itself."""
    kinematic = True

    def __init__(self, num_envs, num_bodies, dof_offsets, dof_limits_lower, dof_limits_upper, body_names, dt=1.0 / 60.0, device='cpu',
                 num_other_actors=0):
        dev = torch.device(device)
        self.num_envs, self.num_bodies, self.dt = int(num_envs), int(num_bodies), float(dt)
        self.dof_offsets = [int(x) for x in dof_offsets]
        self.num_dof = self.dof_offsets[-1]
        self.dof_limits_lower, self.dof_limits_upper = dof_limits_lower, dof_limits_upper
        self.motor_efforts = torch.zeros(self.num_dof, dtype=torch.float32, device=dev)
        self._body_names = list(body_names)
        n, B, D = self.num_envs, self.num_bodies, self.num_dof
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.root_states, self.dof_state = z(n, 1 + int(num_other_actors), 13), z(n, D, 2)
        self.rigid_body_state, self.contact_forces = z(n, B, 13), z(n, B, 3)
        self.root_states[..., 6] = 1.0                        # identity rotations until the first sync
        self.rigid_body_state[..., 6] = 1.0
        rb = self.rigid_body_state
        self.state = {'rigid_body_pos': rb[:, :, 0:3], 'rigid_body_rot': rb[:, :, 3:7], 'rigid_body_vel': rb[:, :, 7:10],
                      'rigid_body_ang_vel': rb[:, :, 10:13], 'dof_pos': self.dof_state[:, :, 0], 'dof_vel': self.dof_state[:, :, 1],
                      'humanoid_root_states': self.root_states[:, 0], 'contact_forces': self.contact_forces}

    def body_ids(self, names):
        return [self._body_names.index(x) for x in names]

    def apply(self, targets, pd):
        pass

    def step(self):
        pass

    def push_state(self, env_ids):
        pass
