"""Device-side resets of ``HumanoidAMP`` / ``HumanoidAMPGetup``: state initialisation of the environments that
just terminated and their AMP observation history - ``_reset_actors`` (``Default`` / ``Start`` / ``Random`` / ``Hybrid``),
``_set_env_state``, ``_init_amp_obs`` (env/tasks/humanoid_amp.py:132-275 of the reference) and the recovery / fall
episodes with the recovery counter of the get-up task (env/tasks/humanoid_amp_getup.py:78-142) - as ONE HIP launch per reset
batch (``ase_hip_amp_reset``, csrc/amp_reset.hip); there is no host fallback.

``HumanoidAMPTensors`` is the sibling of ``env_tensors.HumanoidTensors``: it owns ``amp_obs_buf`` [N, S, F] (and
``recovery_counter`` with the get-up options) and takes the simulator's tensors as the same ``state`` dict plus ``dof_pos`` /
``dof_vel`` [N, D] - plain tensors or the two views of the simulator's interleaved [N, D, 2] dof state.  A reset is a draw
(``draw_reset`` -> a plan of device tensors) and an apply (``apply_reset``: the launch), so that a recorded plan can be applied
and an apply can be recorded in a launch program.  Binding a simulator (pushing the written state to the physics engine)
and ``_generate_fall_states`` (which needs physics) stay with the caller; the target resets of the four tasks are
``env_tensors.HumanoidTensors.reset_task`` - for the strike task called after ``apply_reset``, as the reference does.

``reset_due`` (N10) is the same reset without the host: ONE launch (``ase_hip_amp_reset_due``) tests ``reset_buf``, draws and
applies, and exports the decisions as a full-length plan whose ``env_ids`` hold -1 where nothing was reset.  The draws of
environment e depend on (seed, stream position, e) only, so a partial reset draws other values than ``draw_reset`` under a
torch generator: the method is separate and opt-in.  The reset sequence of a step then makes no torch op that waits for the
host (``tensors``: the ``HumanoidTensors`` of the task, ``amp``: this class, ``agent``: an ``ASEAgent``)::

    reset_buf, terminate_buf = tensors.compute_reset(state, progress_buf)
    amp.mask_recovery(reset_buf, terminate_buf)
    plan = amp.reset_due(state, progress_buf, reset_buf, terminate_buf)
    tensors.reset_task(state, plan['env_ids'], progress_buf)           # skips the -1 rows
    backend.latent_renew(latents, env_ids=plan['env_ids'], rng_state=agent_rng_state, reset_steps=latent_reset_steps,
                         steps_low=latent_steps_min, steps_high=latent_steps_max)
"""
import numpy as np
import torch

from . import lib as L

STATE_INIT = ('Default', 'Start', 'Random', 'Hybrid')        # HumanoidAMP.StateInit (humanoid_amp.py:17-21)


class HumanoidAMPTensors:
    def __init__(self, backend, motion_lib, num_envs, num_amp_obs_steps=10, dt=1.0 / 30.0, state_init='Random', hybrid_init_prob=0.5,
                 local_root_obs=True, root_height_obs=True, recovery_episode_prob=None, recovery_steps=None, fall_init_prob=None,
                 generator=None, device=None, seed=0):
        if state_init not in STATE_INIT:
            raise ValueError(f"state_init must be one of {STATE_INIT}, got {state_init!r}")
        getup = (recovery_episode_prob, recovery_steps, fall_init_prob)
        if any(o is not None for o in getup) and any(o is None for o in getup):
            raise ValueError("the get-up task needs recovery_episode_prob, recovery_steps AND fall_init_prob")
        self.be, self._motion_lib, self.gen = backend, motion_lib, generator
        self.num_envs, self._num_amp_obs_steps, self.dt = int(num_envs), int(num_amp_obs_steps), float(dt)
        self._state_init, self._hybrid_init_prob = state_init, float(hybrid_init_prob)
        self._local_root_obs, self._root_height_obs = bool(local_root_obs), bool(root_height_obs)
        self.getup = recovery_steps is not None
        if self.getup:
            self._recovery_episode_prob, self._fall_init_prob = float(recovery_episode_prob), float(fall_init_prob)
            self._recovery_steps = int(recovery_steps)
        dev = torch.device(device if device is not None else getattr(backend, 'device', 'cpu'))
        self.device = dev
        c = motion_lib.clips
        self._dof_offsets, self._key_body_ids = c['dof_offsets'], c['key_body_ids']
        n_joints = len(self._dof_offsets) - 1
        # [root_h, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos] (humanoid_amp.py:107-118)
        self._num_amp_obs_per_step = 13 + 6 * n_joints + self._dof_offsets[-1] + 3 * len(self._key_body_ids)
        self.amp_obs_buf = torch.zeros(self.num_envs, self._num_amp_obs_steps, self._num_amp_obs_per_step, dtype=torch.float32, device=dev)
        self.recovery_counter = torch.zeros(self.num_envs, dtype=torch.int32, device=dev) if self.getup else None
        self._initial, self._fall, self._table = None, None, None
        # reset_due: the Philox {seed, offset} of the device-side draws and the plan it exports, one element per environment
        self.rng_state = torch.tensor([int(seed), 0], dtype=torch.int64, device=dev)
        self.plan = {k: torch.zeros(self.num_envs, dtype=torch.float32 if k == 'motion_times' else torch.int32, device=dev)
                     for k in ('env_ids', 'kind', 'motion_ids', 'motion_times', 'src_rows')}

    def get_num_amp_obs(self):
        """humanoid_amp.py:61-62."""
        return self._num_amp_obs_steps * self._num_amp_obs_per_step

    # ---- state tables: one table for the launch, the initial state in rows [0, N), the fall states behind it
    def _set_table(self):
        parts = [t for t in (self._initial, self._fall) if t is not None]
        self._table = tuple(torch.cat([p[i] for p in parts]).contiguous() for i in range(3))

    def _as_table(self, root_states, dof_pos, dof_vel):
        t = tuple(torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous() for x in (root_states, dof_pos, dof_vel))
        D = self._dof_offsets[-1]
        if t[0].dim() != 2 or t[0].shape[1] != 13 or t[1].shape != (t[0].shape[0], D) or t[2].shape != t[1].shape:
            raise ValueError("a state table is root_states [T, 13], dof_pos [T, D], dof_vel [T, D]")
        return t

    def set_initial_state(self, root_states, dof_pos, dof_vel):
        """``_initial_humanoid_root_states`` / ``_initial_dof_pos`` / ``_initial_dof_vel``: one row per environment."""
        t = self._as_table(root_states, dof_pos, dof_vel)
        if t[0].shape[0] != self.num_envs:
            raise ValueError("the initial state has one row per environment")
        self._initial = t
        self._set_table()

    def set_fall_states(self, root_states, dof_pos, dof_vel):
        """``_fall_root_states`` / ``_fall_dof_pos`` / ``_fall_dof_vel`` as ``_generate_fall_states`` left them (any row count)."""
        if self._initial is None:
            raise ValueError("set_initial_state comes first (the fall states sit behind it in the table)")
        self._fall = self._as_table(root_states, dof_pos, dof_vel)
        self._set_table()

    # ---- the draw
    def _bernoulli(self, p, n):
        return torch.bernoulli(torch.full((n,), p, dtype=torch.float32, device=self.device), generator=self.gen) == 1.0

    def _draw_ref(self, plan, rows):
        """``_reset_ref_state_init`` (humanoid_amp.py:160-186) for the rows of the plan in the bool mask `rows`."""
        n = int(rows.sum())
        if n == 0:
            return
        ml = self._motion_lib
        motion_ids = ml.sample_motions(n).to(self.device)
        if self._state_init == 'Start':
            motion_times = torch.zeros(n, dtype=torch.float32, device=self.device)
        else:
            motion_times = ml.sample_time(motion_ids).to(self.device)
        plan['kind'][rows] = L.RESET_MOTION
        plan['motion_ids'][rows] = motion_ids.to(torch.int32)
        plan['motion_times'][rows] = motion_times.to(torch.float32)

    def _draw_default(self, plan, rows):
        """``_reset_default`` (humanoid_amp.py:153-158): row e of the initial state."""
        if self._initial is None:
            raise ValueError("Default / Hybrid state initialisation needs set_initial_state")
        plan['kind'][rows] = L.RESET_TABLE
        plan['src_rows'][rows] = plan['env_ids'][rows]

    def _draw_actors(self, plan, rows):
        """``HumanoidAMP._reset_actors`` (humanoid_amp.py:141-201)."""
        if self._state_init == 'Default':
            self._draw_default(plan, rows)
        elif self._state_init in ('Start', 'Random'):
            self._draw_ref(plan, rows)
        else:
            ref = rows.clone()
            ref[rows] = self._bernoulli(self._hybrid_init_prob, int(rows.sum()))
            self._draw_ref(plan, ref)
            self._draw_default(plan, rows & ~ref)

    def draw_reset(self, env_ids, terminate_buf=None):
        """The random part of ``_reset_actors``: which row is reset how -> plan, a dict of device tensors of one element per
        env_id (``env_ids, kind, src_rows, motion_ids`` int32, ``motion_times`` f32; kinds: lib.RESET_*).  With the get-up
        options the three-way split of humanoid_amp_getup.py:78-103: a recovery episode (the state stays, kind RESET_FRAME)
        only for rows with ``terminate_buf == 1``, else a fall state (RESET_TABLE, a row behind the initial state), else
        the underlying state initialisation.  env_ids must be distinct."""
        dev = self.device
        ids = torch.as_tensor(env_ids, device=dev).long().view(-1)
        n = ids.numel()
        plan = {'env_ids': ids.to(torch.int32), 'kind': torch.zeros(n, dtype=torch.int32, device=dev),
                'motion_ids': torch.zeros(n, dtype=torch.int32, device=dev), 'motion_times': torch.zeros(n, dtype=torch.float32, device=dev),
                'src_rows': torch.zeros(n, dtype=torch.int32, device=dev)}
        rows = torch.ones(n, dtype=torch.bool, device=dev)
        if self.getup and n > 0:
            if terminate_buf is None:
                raise ValueError("the get-up task draws recovery episodes from terminate_buf")
            recovery = self._bernoulli(self._recovery_episode_prob, n) & (terminate_buf[ids] == 1)
            plan['kind'][recovery] = L.RESET_FRAME
            rows = ~recovery
            fall = rows.clone()
            fall[rows] = self._bernoulli(self._fall_init_prob, int(rows.sum()))
            n_fall = int(fall.sum())
            if n_fall > 0:
                if self._fall is None:
                    raise ValueError("fall episodes need set_fall_states")
                fall_state_ids = torch.randint(0, self._fall[0].shape[0], (n_fall,), device=dev, generator=self.gen)
                plan['kind'][fall] = L.RESET_TABLE
                plan['src_rows'][fall] = (fall_state_ids + self.num_envs).to(torch.int32)
            rows = rows & ~fall
        if n > 0:
            self._draw_actors(plan, rows)
        return plan

    # ---- the apply
    def _launch(self, state, plan, kinds):
        s = state
        self.be.amp_reset(self._motion_lib.clips, plan['env_ids'], plan['kind'], plan.get('motion_ids'), plan.get('motion_times'),
                          plan.get('src_rows'), self._table, s['humanoid_root_states'], s['dof_pos'], s['dof_vel'], s['rigid_body_pos'],
                          s['rigid_body_rot'], s['rigid_body_vel'], s['rigid_body_ang_vel'], self._local_root_obs,
                          self._root_height_obs, self.dt, self.amp_obs_buf, kinds)

    def apply_reset(self, state, plan, progress_buf=None, reset_buf=None, terminate_buf=None):
        """``_reset_actors`` + ``_init_amp_obs`` of the plan's rows in one launch, then ``_reset_env_tensors``' three row fills
        (humanoid.py:165-167) and the recovery counter (humanoid_amp_getup.py:101,106,114).  The plan's tensors are read when
        the launch runs; while a launch program records, the torch part is recorded with it."""
        if plan['env_ids'].numel() == 0:
            return
        self._launch(state, plan, L.RESET_HAS_MOTION | (L.RESET_HAS_TABLE if self._table is not None else 0))

        def env_tensors():
            ids = plan['env_ids'].long()
            for buf in (progress_buf, reset_buf, terminate_buf):
                if buf is not None:
                    buf.index_fill_(0, ids, 0)
            if self.getup:
                kind, src = plan['kind'], plan['src_rows']
                counted = (kind == L.RESET_FRAME) | ((kind == L.RESET_TABLE) & (src >= self.num_envs))
                steps = torch.where(counted, self._recovery_steps, 0).to(torch.int32)
                self.recovery_counter.index_copy_(0, ids, steps)
        self.be.host_call(env_tensors)

    def reset(self, state, env_ids, progress_buf=None, reset_buf=None, terminate_buf=None):
        """``_reset_envs`` (humanoid_amp.py:132-139) without the simulator calls: the draw and the apply -> the plan."""
        plan = self.draw_reset(env_ids, terminate_buf)
        self.apply_reset(state, plan, progress_buf, reset_buf, terminate_buf)
        return plan

    def reset_due(self, state, progress_buf, reset_buf, terminate_buf=None, advance=True):
        """``_reset_envs`` for every environment with ``reset_buf != 0``, due test, draws, apply and ``_reset_env_tensors`` in
        ONE launch (``ase_hip_amp_reset_due``; the draw table is in include/ase_hip.h) -> ``self.plan``: five [N] device
        tensors that the launch fills, ``env_ids`` = e for a reset environment and -1 otherwise - a valid plan of
        ``apply_reset`` and an id list for ``HumanoidTensors.reset_task`` / ``latent_renew``, which skip -1.  No torch op, no
        ``host_call``, no synchronisation: it can be recorded in a launch program and follows the buffers at replay.
        ``rng_state`` moves on by one unless advance is false.  The clip of a motion row comes from ``DeviceMotionLib.clip_cdf``."""
        if self.getup and terminate_buf is None:
            raise ValueError("the get-up task draws recovery episodes from terminate_buf")
        init = STATE_INIT.index(self._state_init)
        if init in (L.INIT_DEFAULT, L.INIT_HYBRID) and self._initial is None:
            raise ValueError("Default / Hybrid state initialisation needs set_initial_state")
        getup = None
        if self.getup:
            if self._fall_init_prob > 0 and self._fall is None:
                raise ValueError("fall episodes need set_fall_states")
            getup = (self._recovery_episode_prob, self._recovery_steps, self._fall_init_prob)
        s, ml = state, self._motion_lib
        self.be.amp_reset_due(ml.clips, ml.clip_cdf, self._table, init, self._hybrid_init_prob, getup, self.rng_state, progress_buf,
                              reset_buf, terminate_buf, self.recovery_counter, self.plan, s['humanoid_root_states'], s['dof_pos'],
                              s['dof_vel'], s['rigid_body_pos'], s['rigid_body_rot'], s['rigid_body_vel'], s['rigid_body_ang_vel'],
                              self._local_root_obs, self._root_height_obs, self.dt, self.amp_obs_buf, advance=advance)
        return self.plan

    def compute_amp_observations(self, state, env_ids):
        """``_compute_amp_observations(env_ids)`` (humanoid_amp.py:267-274): slot 0 of those rows, nothing else."""
        ids = torch.as_tensor(env_ids, device=self.device).to(torch.int32).contiguous().view(-1)
        if ids.numel():
            self._launch(state, {'env_ids': ids, 'kind': torch.zeros_like(ids)}, 0)

    def post_physics_step(self, state):
        """``_update_hist_amp_obs`` + ``_compute_amp_observations`` for every environment (humanoid_amp.py:50-59) -> the flat
        [N, S * F] view (``extras["amp_obs"]``)."""
        s = state
        root = lambda k: s[k][:, 0].contiguous()
        self.be.build_amp_obs(root('rigid_body_pos'), root('rigid_body_rot'), root('rigid_body_vel'), root('rigid_body_ang_vel'),
                              s['dof_pos'].contiguous(), s['dof_vel'].contiguous(), s['rigid_body_pos'][:, self._key_body_ids].contiguous(),
                              self._dof_offsets, self._local_root_obs, self._root_height_obs, self.amp_obs_buf, shift=True)
        return self.amp_obs_buf.view(self.num_envs, self.get_num_amp_obs())

    # ---- the recovery counter of the get-up task
    def pre_physics_step(self):
        """``_update_recovery_count`` (humanoid_amp_getup.py:131-134)."""
        if self.getup:
            self.recovery_counter.sub_(1).clamp_min_(0)

    def mask_recovery(self, reset_buf, terminate_buf):
        """``HumanoidAMPGetup._compute_reset`` after the base test (humanoid_amp_getup.py:136-142): no reset and no
        termination while an environment recovers."""
        if self.getup:
            is_recovery = self.recovery_counter > 0
            reset_buf.masked_fill_(is_recovery, 0)
            terminate_buf.masked_fill_(is_recovery, 0)
        return reset_buf, terminate_buf


def pd_action_offset_scale(dof_limits_lower, dof_limits_upper, dof_offsets):
    """``_build_pd_action_offset_scale`` (env/tasks/humanoid.py:314-359), host, run once: 3-dof joints get a symmetric range of
    1.2 x their largest limit (at most pi), hinges 0.7 x their span about the middle -> (offset, scale), f32 [D]."""
    lim_low = torch.as_tensor(dof_limits_lower).detach().cpu().numpy().copy()
    lim_high = torch.as_tensor(dof_limits_upper).detach().cpu().numpy().copy()
    for j in range(len(dof_offsets) - 1):
        o, size = dof_offsets[j], dof_offsets[j + 1] - dof_offsets[j]
        if size == 3:
            curr_low = np.max(np.abs(lim_low[o:o + size]))
            curr_high = np.max(np.abs(lim_high[o:o + size]))
            curr_scale = min([1.2 * max([curr_low, curr_high]), np.pi])
            lim_low[o:o + size] = -curr_scale
            lim_high[o:o + size] = curr_scale
        elif size == 1:
            curr_low, curr_high = lim_low[o], lim_high[o]
            curr_mid = 0.5 * (curr_high + curr_low)
            # a bit beyond the joint limits, so that the motors keep their strength near them
            curr_scale = 0.7 * (curr_high - curr_low)
            lim_low[o] = curr_mid - curr_scale
            lim_high[o] = curr_mid + curr_scale
    offset, scale = 0.5 * (lim_high + lim_low), 0.5 * (lim_high - lim_low)
    return torch.tensor(offset, dtype=torch.float32), torch.tensor(scale, dtype=torch.float32)


def action_to_pd_targets(action, pd_action_offset, pd_action_scale):
    """``_action_to_pd_targets`` (env/tasks/humanoid.py:479-481)."""
    return pd_action_offset + pd_action_scale * action
