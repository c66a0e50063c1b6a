"""The humanoid task environment on the device: the step and reset logic of the reference's ``Humanoid``,
``HumanoidAMP``, ``HumanoidAMPGetup``, ``HumanoidHeading``, ``HumanoidLocation``, ``HumanoidReach``, ``HumanoidStrike`` and
``HumanoidPerturb`` (env/tasks/humanoid.py:361-383, humanoid_amp.py:50-59,132-139, humanoid_amp_getup.py:63-66,131-142,
humanoid_perturb.py:149-167,172-213, base/vec_task.py:90-118 of the reference) as ONE class on a small physics protocol.
``HumanoidEnv`` composes ``env_tensors.HumanoidTensors``, ``amp_env.HumanoidAMPTensors``, ``amp_env.pd_action_offset_scale``,
``motion_lib.DeviceMotionLib`` / ``AmpObsDemoSource`` and ``perturb.ProjectileLauncher`` and exposes what the agents and players
use of an environment (the interface of ``synthetic.SyntheticVecEnv``).

One step is::

    env_pre_step   (one launch)   action clamp + copy, PD targets / forces, prev_root_pos, recovery counter
    update_task    (one launch)   the task's due targets are redrawn (it draws, so it is a launch of its own)
    physics.apply(targets, pd); physics.step()
    proj_launch    (one launch)   perturb only: the projectile that is due by progress_buf[0] is launched (it draws too)
    env_post_step  (one launch)   progress, observation, reward, reset / terminate, AMP history, observation clip

Both launches read the simulator's tensors in place, at their own strides.  With ``fused_step=False`` the same step is made
with the separate methods of ``HumanoidTensors`` / ``HumanoidAMPTensors`` and torch glue: the composition the fused step is
tested against, bit for bit.

The physics protocol - what an Isaac-Gym-like binding supplies:

    num_envs, num_bodies, num_dof, dt       sizes and the control step (seconds)
    dof_offsets                             python list, joint j owns dofs [dof_offsets[j], dof_offsets[j + 1])
    dof_limits_lower / dof_limits_upper     [num_dof]
    motor_efforts                           f32 [num_dof] on the device (torque control)
    body_ids(names) -> list of int          rigid-body indices of the named bodies
    state                                   dict of device tensors, strided views allowed: rigid_body_pos / _vel / _ang_vel
                                            [n, B, 3], rigid_body_rot [n, B, 4], contact_forces [n, B, 3], humanoid_root_states
                                            [n, 13], dof_pos / dof_vel [n, D]; for strike target_states [n, 13] and
                                            tar_contact_forces [n, 3]
    apply(targets, pd)                      targets f32 [n, D]: PD position targets (pd) or forces
    step()                                  the substeps and the refresh of the state tensors
    push_state(env_ids)                     the indexed set calls (root and dof state) for int32 env_ids; a full-length list
                                            with -1 for "skip" must be accepted, so the device reset path needs no compaction
    state['proj_states']                    perturb only: [n, K, 13], the projectiles' rows of the root-state tensor
    push_projectiles(env_ids, slot)         perturb only: the indexed root-state set call for the projectiles of int32 env_ids
                                            (-1: skip); slot is a device int32 word that holds the one projectile to push, or
                                            -1 for none, and None stands for all projectiles of those environments

``PlaybackPhysics`` is the stand-in of the tests and the benchmark: it replays recorded frames in the packed simulator layout
and invents no dynamics.  A real simulator binding, ``_generate_fall_states``, ``_update_marker``,
the ``dr_randomizations`` hooks and rendering are out of scope (``humanoid_view_motion`` is ``ase_amd/view_motion.py``).

``perturb=True`` (or a dict of ``perturb.ProjectileLauncher`` arguments) makes the environment the reference's
``HumanoidPerturb``: a HumanoidAMP whose ``post_physics_step`` first launches the projectile that is due - by the counter of
environment 0, for all environments, as the reference does - and whose reset test is the timeout alone.
"""
import math

import torch

from .amp_env import HumanoidAMPTensors, action_to_pd_targets, pd_action_offset_scale
from .env_tensors import HumanoidTensors
from .motion_lib import AmpObsDemoSource
from .perturb import ProjectileLauncher
from .synthetic import _Space

BODY_KEYS = ('rigid_body_pos', 'rigid_body_rot', 'rigid_body_vel', 'rigid_body_ang_vel')

# env_cfg keys -> HumanoidTensors' reset parameters, per task
TASK_KEYS = {
    None: {},
    'heading': dict(tarSpeedMin='tar_speed_min', tarSpeedMax='tar_speed_max', headingChangeStepsMin='heading_change_steps_min',
                    headingChangeStepsMax='heading_change_steps_max', enableRandHeading='enable_rand_heading'),
    'location': dict(tarSpeed='tar_speed', tarChangeStepsMin='tar_change_steps_min', tarChangeStepsMax='tar_change_steps_max',
                     tarDistMax='tar_dist_max'),
    'reach': dict(tarSpeed=None, tarChangeStepsMin='tar_change_steps_min', tarChangeStepsMax='tar_change_steps_max',
                  tarDistMax='tar_dist_max', tarHeightMin='tar_height_min', tarHeightMax='tar_height_max', reachBodyName=None),
    'strike': dict(strikeBodyNames=None),
}
COMMON_KEYS = ('numEnvs', 'episodeLength', 'localRootObs', 'enableEarlyTermination', 'pdControl', 'powerScale', 'stateInit',
               'hybridInitProb', 'numAMPObsSteps', 'keyBodies', 'contactBodies', 'terminationHeight', 'enableTaskObs')
GETUP_KEYS = ('recoveryEpisodeProb', 'recoverySteps', 'fallInitProb')
OFF_KEYS = ('enableDebugVis', 'isFlagrun')           # accepted only when false: the class has no viewer and no flag run


class HumanoidEnv:
    resets_done_on_device = True      # reset_done(mask): what the agents' device_rollout asks of an environment

    def __init__(self, backend, physics, env_cfg, motion_lib=None, task=None, getup=False, fused_step=True, seed=0,
                 clip_observations=5.0, clip_actions=1.0, perturb=None):
        """env_cfg: the ``env`` section of the reference's task yaml (its key names).  motion_lib: a ``DeviceMotionLib`` - with
        it the environment is a HumanoidAMP (history, demo fetch, reference state initialisation), without it the plain
        Humanoid.  clip_observations / clip_actions: the task config's values (5.0 / 1.0 in the reference).  perturb: None, True
        or a dict of ``ProjectileLauncher`` arguments - the HumanoidPerturb class: projectiles on the reference's schedule, reset
        by timeout only (its own compute_humanoid_reset ignores enableEarlyTermination)."""
        if task not in TASK_KEYS:
            raise ValueError(f"task must be one of {list(TASK_KEYS)}, got {task!r}")
        if perturb is not None and perturb is not True and not isinstance(perturb, dict):
            raise ValueError(f"perturb must be None, True or a dict of ProjectileLauncher arguments, got {perturb!r}")
        if perturb is not None and (task is not None or getup):
            raise ValueError("perturb is the reference's HumanoidPerturb: no task and no get-up episodes combine with it")
        if perturb is not None and motion_lib is None:
            raise ValueError("the perturbation task is a HumanoidAMP: it needs a motion_lib")
        cfg = dict(env_cfg)
        known = set(COMMON_KEYS) | set(TASK_KEYS[task]) | set(OFF_KEYS) | (set(GETUP_KEYS) if getup else set())
        unknown = sorted(set(cfg) - known)
        if unknown:
            raise ValueError(f"HumanoidEnv(task={task!r}, getup={getup}) does not implement the env keys {unknown} "
                             "(the simulator's own keys belong to the physics binding)")
        for k in OFF_KEYS:
            if cfg.get(k, False):
                raise ValueError(f"HumanoidEnv does not implement {k}")
        if getup and motion_lib is None:
            raise ValueError("the get-up task is a HumanoidAMP: it needs a motion_lib")
        missing = [k for k in GETUP_KEYS if getup and k not in cfg]
        if missing:
            raise ValueError(f"the get-up task needs the env keys {missing}")
        self.be, self.physics, self.fused_step = backend, physics, bool(fused_step)
        ph = physics
        n = self.num_envs = int(ph.num_envs)
        if int(cfg.get('numEnvs', n)) != n:
            raise ValueError(f"numEnvs {cfg['numEnvs']} but the physics has {n} environments")
        self.device = torch.device(getattr(backend, 'device', 'cpu'))
        dev = self.device
        state = ph.state
        if task == 'strike' and not ('target_states' in state and 'tar_contact_forces' in state):
            raise ValueError("the strike task needs target_states and tar_contact_forces in physics.state")
        self.task_name, self.getup = task, bool(getup)
        self.launcher = None
        if perturb is not None:
            kw = dict(seed=seed + 3)
            kw.update(perturb if isinstance(perturb, dict) else {})
            self.launcher = ProjectileLauncher(backend, n, device=dev, **kw)
            proj = state.get('proj_states')
            if proj is None or proj.dim() != 3 or proj.shape[0] != n or proj.shape[2] != 13 or proj.shape[1] < self.launcher.n_slots:
                raise ValueError(f"perturb needs physics.state['proj_states'] [{n}, >= {self.launcher.n_slots}, 13]"
                                 + ("" if proj is None else f", got {tuple(proj.shape)}"))
            if not callable(getattr(ph, 'push_projectiles', None)):
                raise ValueError("perturb needs physics.push_projectiles(env_ids, slot)")
        self.clip_obs, self.clip_actions = float(clip_observations), float(clip_actions)
        self._pd_control, self._power_scale = bool(cfg.get('pdControl', True)), float(cfg.get('powerScale', 1.0))
        self._enable_task_obs = bool(cfg.get('enableTaskObs', True)) and task is not None
        B, D = int(ph.num_bodies), int(ph.num_dof)
        task_kw = {v: cfg[k] for k, v in TASK_KEYS[task].items() if v is not None and k in cfg}
        if task == 'strike':
            task_kw['strike_body_ids'] = ph.body_ids(cfg['strikeBodyNames'])
        if task == 'reach':
            task_kw['reach_body_id'] = ph.body_ids([cfg['reachBodyName']])[0]
        self.tensors = HumanoidTensors(backend, n, B, task=task, local_root_obs=cfg.get('localRootObs', True),
                                       contact_body_ids=ph.body_ids(cfg.get('contactBodies', [])),
                                       termination_heights=cfg.get('terminationHeight', 0.15),
                                       max_episode_length=cfg.get('episodeLength', 300),
                                       enable_early_termination=cfg.get('enableEarlyTermination', True) and perturb is None,
                                       dt=ph.dt, device=dev,
                                       seed=seed, **task_kw)
        self.amp = None
        if motion_lib is not None:
            clips = motion_lib.clips
            if list(clips['dof_offsets']) != [int(x) for x in ph.dof_offsets]:
                raise ValueError("the motion library's dof_offsets are not the physics'")
            if 'keyBodies' in cfg and ph.body_ids(cfg['keyBodies']) != [int(x) for x in clips['key_body_ids']]:
                raise ValueError("keyBodies are not the motion library's key bodies")
            gk = dict(recovery_episode_prob=cfg['recoveryEpisodeProb'], recovery_steps=cfg['recoverySteps'],
                      fall_init_prob=cfg['fallInitProb']) if getup else {}
            self.amp = HumanoidAMPTensors(backend, motion_lib, n, num_amp_obs_steps=cfg.get('numAMPObsSteps', 10), dt=ph.dt,
                                          state_init=cfg.get('stateInit', 'Random'), hybrid_init_prob=cfg.get('hybridInitProb', 0.5),
                                          local_root_obs=cfg.get('localRootObs', True), device=dev, seed=seed + 1, **gk)
            self.demo_source = AmpObsDemoSource(motion_lib, backend, num_amp_obs_steps=cfg.get('numAMPObsSteps', 10), dt=ph.dt,
                                                local_root_obs=cfg.get('localRootObs', True), seed=seed + 2)
        self._fall_prob = float(cfg['fallInitProb']) if getup else 0.0
        off, scale = pd_action_offset_scale(ph.dof_limits_lower, ph.dof_limits_upper, ph.dof_offsets)
        self._pd_offset, self._pd_scale = off.to(dev), scale.to(dev)
        self.progress_buf = torch.zeros(n, dtype=torch.int64, device=dev)
        self.actions = torch.zeros(n, D, dtype=torch.float32, device=dev)
        self.targets = torch.zeros(n, D, dtype=torch.float32, device=dev)
        self.prev_root_pos = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        self._task_state = self._alloc_targets(task, n, dev)
        self.obs_buf, self.rew_buf = self.tensors.obs_buf, self.tensors.rew_buf
        self.reset_buf, self.terminate_buf = self.tensors.reset_buf, self.tensors.terminate_buf
        if task is not None and not self._enable_task_obs:       # the task columns stay out of the observation
            self.obs_buf = self.tensors.obs_buf[:, :self.tensors.get_humanoid_obs_size()]
        self.observation_space = _Space(self.obs_buf.shape[1], low=-math.inf, high=math.inf)
        self.action_space = _Space(D)
        self.amp_observation_space = _Space(self.amp.get_num_amp_obs()) if self.amp is not None else None
        self.env = self.task = self
        self.viewer = None
        self._shadow = None

    @staticmethod
    def _alloc_targets(task, n, dev):
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        if task == 'heading':
            t = {'tar_dir': z(n, 2), 'tar_facing_dir': z(n, 2), 'tar_speed': torch.ones(n, dtype=torch.float32, device=dev)}
            t['tar_dir'][:, 0] = 1.0
            t['tar_facing_dir'][:, 0] = 1.0
            return t
        if task == 'location':
            return {'tar_pos': z(n, 2)}
        if task == 'reach':
            return {'tar_pos': z(n, 3)}
        return {}

    # ---- the state the tensor classes read: the physics' tensors plus the environment's own
    @property
    def state(self):
        s = dict(self.physics.state)
        s.update(self._task_state)
        s['prev_root_pos'] = self.prev_root_pos
        return s

    def set_initial_state(self, root_states, dof_pos, dof_vel):
        self.amp.set_initial_state(root_states, dof_pos, dof_vel)

    def set_fall_states(self, root_states, dof_pos, dof_vel):
        self.amp.set_fall_states(root_states, dof_pos, dof_vel)

    def get_task_obs_size(self):
        return self.tensors.get_task_obs_size() if self._enable_task_obs else 0

    def fetch_amp_obs_demo(self, n):
        return self.demo_source.fetch_amp_obs_demo(n)

    def fetch_amp_obs_demo_into(self, data, ring_rows, head, n):
        self.demo_source.fetch_into(data, ring_rows, head, n)

    # ---- resets.  The reset entries take contiguous rigid-body tensors: where the physics hands out windows of a packed
    # tensor they work on a contiguous shadow that is copied in and written back
    def _contiguous_state(self):
        s = self.state
        if all(s[k].is_contiguous() for k in BODY_KEYS):
            return s, None
        if self._shadow is None:
            self._shadow = {k: torch.empty(s[k].shape, dtype=torch.float32, device=self.device) for k in BODY_KEYS}
        for k in BODY_KEYS:
            self._shadow[k].copy_(s[k])
        packed = {k: s[k] for k in BODY_KEYS}
        s.update(self._shadow)
        return s, packed

    def _write_back(self, packed):
        if packed is not None:
            for k in BODY_KEYS:
                packed[k].copy_(self._shadow[k])

    def _clipped_obs(self):
        return torch.clamp(self.obs_buf, -self.clip_obs, self.clip_obs)

    def _compute_observations(self, s, ids):
        t = self.tensors
        self.be.humanoid_obs_max(s['rigid_body_pos'], s['rigid_body_rot'], s['rigid_body_vel'], s['rigid_body_ang_vel'],
                                 t.local_root_obs, t.root_height_obs, t.obs_buf, 0, ids)
        if self._enable_task_obs:
            ops = {k: v.contiguous() for k, v in t._task_operands(s).items()}        # (actor windows of the packed root tensor)
            self.be.task_obs(t.kind, t.obs_buf, t.get_humanoid_obs_size(), ids, **ops)

    def _check_fall(self):
        if self.getup and self._fall_prob > 0 and self.amp._fall is None:
            raise ValueError("fallInitProb > 0 needs set_fall_states (the fall states come from the physics binding)")

    def reset(self, env_ids=None):
        """The host path (``_reset_envs`` + ``VecTaskPython.reset``): ``amp.reset``, ``reset_task``, ``push_state``, then the
        observation of those rows -> the clipped observation."""
        self._check_fall()
        ids = torch.arange(self.num_envs, device=self.device) if env_ids is None else torch.as_tensor(env_ids, device=self.device).view(-1)
        ids = ids.to(torch.int32).contiguous()
        if ids.numel() > 0:
            s, packed = self._contiguous_state()
            if self.amp is not None:
                self.amp.reset(s, ids, self.progress_buf, self.reset_buf, self.terminate_buf)
            else:
                for buf in (self.progress_buf, self.reset_buf, self.terminate_buf):
                    buf.index_fill_(0, ids.long(), 0)
            self.tensors.reset_task(s, ids, self.progress_buf)
            self._write_back(packed)
            self.physics.push_state(ids)
            if self.launcher is not None:
                self.physics.push_projectiles(ids, None)
            self._compute_observations(s, ids)
        return self._clipped_obs()

    def reset_done(self, mask=None):
        """The device path: ``amp.reset_due`` on the environment's own ``reset_buf``, ``reset_task`` and ``push_state`` on the
        plan's full-length id list (-1: skipped), then the observation of those rows.  The host learns nothing.  mask is the
        agent's done mask of the step - the same rows as ``reset_buf``, which the step wrote and the launch tests."""
        if self.amp is None:
            raise ValueError("reset_done is the HumanoidAMP device reset: it needs a motion_lib")
        self._check_fall()
        s, packed = self._contiguous_state()
        plan = self.amp.reset_due(s, self.progress_buf, self.reset_buf, self.terminate_buf)
        self.tensors.reset_task(s, plan['env_ids'], self.progress_buf)
        self._write_back(packed)
        self.physics.push_state(plan['env_ids'])
        if self.launcher is not None:
            self.physics.push_projectiles(plan['env_ids'], None)
        self._compute_observations(s, plan['env_ids'])
        return self._clipped_obs()

    # ---- one step
    def _post_operands(self):
        """Keyword operands of env_post_step for this task."""
        t, s = self.tensors, self.state
        kw = dict(task_kind=t.kind, enable_task_obs=self._enable_task_obs)
        if t.task in ('heading', 'location', 'strike'):
            kw.update(root_states=s['humanoid_root_states'], prev_root_pos=self.prev_root_pos, dt=t.dt)
        if t.task == 'heading':
            kw.update(tar_a=s['tar_dir'], tar_b=s['tar_facing_dir'], tar_speed=s['tar_speed'])
        elif t.task == 'location':
            kw.update(tar_a=s['tar_pos'], tar_speed=t.tar_speed)
        elif t.task == 'reach':
            kw.update(tar_a=s['tar_pos'], reach_body_id=t.reach_body_id)
            if self._enable_task_obs:
                kw.update(root_states=s['humanoid_root_states'])
        elif t.task == 'strike':
            kw.update(tar_states=s['target_states'], tar_contact_forces=s['tar_contact_forces'], strike_body_ids=t.strike_body_ids)
        if self.amp is not None:
            a = self.amp
            kw.update(hist=a.amp_obs_buf, dof_pos=s['dof_pos'], dof_vel=s['dof_vel'], dof_offsets=a._dof_offsets,
                      key_body_ids=a._key_body_ids, recovery_counter=a.recovery_counter)
        return kw

    def pre_physics_step(self, actions):
        t, s = self.tensors, self.state
        prev = self.prev_root_pos if t.task in ('heading', 'location', 'strike') else None
        counter = self.amp.recovery_counter if self.amp is not None else None
        if self.fused_step:
            pd = dict(pd_offset=self._pd_offset, pd_scale=self._pd_scale) if self._pd_control else dict(motor_efforts=self.physics.motor_efforts)
            self.be.env_pre_step(actions, self.actions, self.targets, self.clip_actions, power_scale=self._power_scale,
                                 root_states=s['humanoid_root_states'] if prev is not None else None, prev_root_pos=prev,
                                 recovery_counter=counter, **pd)
        else:
            self.actions.copy_(torch.clamp(actions, -self.clip_actions, self.clip_actions))
            if self._pd_control:
                self.targets.copy_(action_to_pd_targets(self.actions, self._pd_offset, self._pd_scale))
            else:
                self.targets.copy_(self.actions * self.physics.motor_efforts.unsqueeze(0) * self._power_scale)
            if prev is not None:
                prev.copy_(s['humanoid_root_states'][:, 0:3])
            if self.amp is not None:
                self.amp.pre_physics_step()
        t.update_task(s, self.progress_buf)

    def post_physics_step(self):
        """-> the observation of the step (clipped).  Fused: the one launch on the physics' tensors as they are; unfused: the
        separate methods on contiguous copies, as a binding of the existing entries has to make them."""
        t, s = self.tensors, self.state
        if self.launcher is not None:                    # _update_proj runs before progress_buf is incremented
            self.launcher.update(s, self.progress_buf)
            self.physics.push_projectiles(self.launcher.launch_ids, self.launcher.slot_word)
        if self.fused_step:
            self.be.env_post_step(s['rigid_body_pos'], s['rigid_body_rot'], s['rigid_body_vel'], s['rigid_body_ang_vel'],
                                  s['contact_forces'], self.progress_buf, t.obs_buf, self.rew_buf, self.reset_buf, self.terminate_buf,
                                  t.termination_heights, t.contact_body_ids, t.max_episode_length, t.enable_early_termination,
                                  t.local_root_obs, t.root_height_obs, clip_obs=self.clip_obs, **self._post_operands())
            return self.obs_buf
        self.progress_buf += 1
        c = dict(s)
        for k in BODY_KEYS + ('contact_forces', 'humanoid_root_states') + (('target_states', 'tar_contact_forces') if t.task == 'strike' else ()):
            c[k] = s[k].contiguous()
        self._compute_observations(c, None)
        t.compute_reward(c)
        t.compute_reset(c, self.progress_buf)
        if self.amp is not None:
            self.amp.mask_recovery(self.reset_buf, self.terminate_buf)
            self.amp.post_physics_step(c)
        return self._clipped_obs()

    def step(self, actions):
        """-> (obs, rewards, dones, infos{'terminate', 'amp_obs'}), as ``VecTaskPython.step`` + ``RLGPUEnv.step`` hand them out."""
        self.pre_physics_step(actions)
        self.physics.apply(self.targets, self._pd_control)
        self.physics.step()
        obs = self.post_physics_step()
        infos = {'terminate': self.terminate_buf}
        if self.amp is not None:
            infos['amp_obs'] = self.amp.amp_obs_buf.view(self.num_envs, self.amp.get_num_amp_obs())
        return obs, self.rew_buf, self.reset_buf, infos


class PlaybackPhysics:
    """The physics stand-in of the tests and the benchmark: ``step()`` copies frame ``t mod T`` of a recording into the state
    tensors, ``apply`` and ``push_state`` record their argument.  frames: dict of [T, n, ...] tensors in the packed simulator
    layout - ``rigid_body_state`` [T, n, bodies_per_env, 13] (position, rotation, velocity, angular velocity),
    ``dof_state`` [T, n, D, 2], ``root_states`` [T, n, actors_per_env, 13], ``contact_forces`` [T, n, bodies_per_env, 3].
    With bodies_per_env = num_bodies + 1 and two actors the last body and the second actor are the strike task's target.
    ``state`` holds windows of the packed tensors: nothing is contiguous but by accident.  With num_projectiles = K > 0 the
    last K actors are the perturbation task's projectiles, ``state['proj_states']``: they start at frame 0's rows and are not
    played back - what a launch wrote persists - and ``push_projectiles`` records its arguments."""

    def __init__(self, frames, num_bodies, dof_offsets, dof_limits_lower, dof_limits_upper, motor_efforts, body_names, dt=1.0 / 30.0,
                 device='cpu', num_projectiles=0):
        dev = torch.device(device)
        self.frames = {k: v.to(torch.float32).to(dev).contiguous() for k, v in frames.items()}
        rb, dof, root, cf = (self.frames[k] for k in ('rigid_body_state', 'dof_state', 'root_states', 'contact_forces'))
        self.T, self.num_envs, self.num_bodies, self.num_dof, self.dt = rb.shape[0], rb.shape[1], int(num_bodies), dof.shape[2], float(dt)
        assert rb.shape[2] >= self.num_bodies and rb.shape[3] == 13 and cf.shape[:3] == rb.shape[:3] and root.shape[3] == 13
        self.dof_offsets = [int(x) for x in dof_offsets]
        self.dof_limits_lower, self.dof_limits_upper = dof_limits_lower, dof_limits_upper
        self.motor_efforts = torch.as_tensor(motor_efforts, dtype=torch.float32).to(dev)
        self._body_names = list(body_names)
        self._packed = {k: torch.empty_like(v[0]) for k, v in self.frames.items()}
        p, B = self._packed, self.num_bodies
        self.state = {'rigid_body_pos': p['rigid_body_state'][:, :B, 0:3], 'rigid_body_rot': p['rigid_body_state'][:, :B, 3:7],
                      'rigid_body_vel': p['rigid_body_state'][:, :B, 7:10], 'rigid_body_ang_vel': p['rigid_body_state'][:, :B, 10:13],
                      'dof_pos': p['dof_state'][:, :, 0], 'dof_vel': p['dof_state'][:, :, 1],
                      'humanoid_root_states': p['root_states'][:, 0], 'contact_forces': p['contact_forces'][:, :B]}
        K = self.num_projectiles = int(num_projectiles)
        assert 0 <= K < root.shape[2], "the projectiles are the last actors behind the humanoid"
        if rb.shape[2] > B and root.shape[2] - K > 1:
            self.state['target_states'] = p['root_states'][:, 1]
            self.state['tar_contact_forces'] = p['contact_forces'][:, B]
        self.t, self.applied, self.pushed = 0, None, []
        self._load(0)
        if K > 0:
            self.state['proj_states'] = p['root_states'][:, root.shape[2] - K:]
            self.state['proj_states'].copy_(root[0, :, root.shape[2] - K:])
            self.pushed_projectiles = []

    def _load(self, t):
        for k, v in self.frames.items():
            if k == 'root_states' and self.num_projectiles > 0:
                A = v.shape[2] - self.num_projectiles
                self._packed[k][:, :A].copy_(v[t % self.T][:, :A])
            else:
                self._packed[k].copy_(v[t % self.T])

    def body_ids(self, names):
        return [self._body_names.index(x) for x in names]

    def apply(self, targets, pd):
        self.applied = (targets, bool(pd))

    def step(self):
        self._load(self.t)
        self.t += 1

    def push_state(self, env_ids):
        self.pushed.append(env_ids)

    def push_projectiles(self, env_ids, slot):
        assert self.num_projectiles > 0, "a physics without projectiles"
        self.pushed_projectiles.append((env_ids, slot))
