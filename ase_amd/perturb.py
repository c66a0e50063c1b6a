"""The projectile launches of the perturbation task on the device: ``HumanoidPerturb._update_proj``
(env/tasks/humanoid_perturb.py:137-147,172-213 of the reference) behind ``ase_hip_proj_launch``.

``ProjectileLauncher`` holds the reference's constants, the schedule table and the stream of the device draws.  ``update`` is
the per-step call: one launch on a fixed grid that tests the schedule on ``progress_buf[0]`` - the reference's semantics, the
counter of environment 0 decides for all environments - draws on the device and writes the due projectile's root-state row
in place.  The host learns nothing; ``slot_word`` and ``launch_ids`` tell the physics binding what to push.  ``launch_ids`` is
written by the calls over all environments only: a call on an ``env_ids`` list updates ``slot_word`` and leaves ``launch_ids`` as
it was - the caller's own list, with ids outside the range skipped, is the id list of that call.

state: a dict of device tensors, strided views allowed - ``humanoid_root_states`` [n, 13], ``rigid_body_pos`` /
``rigid_body_vel`` [n, B, 3], ``proj_states`` [n, K, 13] (the last K actors of the simulator's root tensor)."""
import torch

# the step counts of the reference's PERTURB_OBJS (humanoid_perturb.py:12-26): object k is launched when the counter, modulo the
# total + 1, equals the sum of the first k + 1 counts
PERTURB_OBJS = (60, 7, 10, 35, 2, 2, 3, 2, 2, 3, 2, 60, 300)
MAX_SLOTS = 32


class ProjectileLauncher:
    def __init__(self, backend, num_envs, objs=PERTURB_OBJS, dist_min=4.0, dist_max=5.0, h_min=0.25, h_max=2.0, speed_min=30.0,
                 speed_max=40.0, noise=0.1, tar_body=1, device=None, seed=0, generator=None):
        """objs: the step counts of the projectiles, in launch order.  generator: the torch generator of ``draw`` (None: the
        global one); seed: the seed of the device-side draws (rng_state)."""
        objs = [int(x) for x in objs]
        if not 1 <= len(objs) <= MAX_SLOTS:
            raise ValueError(f"1 .. {MAX_SLOTS} projectiles, got {len(objs)}")
        if any(x <= 0 for x in objs):
            raise ValueError(f"the step counts must be positive (a strictly increasing schedule), got {objs}")
        total, steps = 0, []
        for x in objs:
            total += x
            steps.append(total)
        if total >= 1 << 31:
            raise ValueError("the schedule does not fit int32")
        self.be, self.num_envs, self.n_slots, self.tar_body = backend, int(num_envs), len(objs), int(tar_body)
        self.objs, self.perturb_timesteps = tuple(objs), tuple(steps)
        self.params = dict(dist_min=dist_min, dist_max=dist_max, h_min=h_min, h_max=h_max, speed_min=speed_min, speed_max=speed_max,
                           noise=noise)
        dev = torch.device(device if device is not None else getattr(backend, 'device', 'cpu'))
        self.device, self.generator = dev, generator
        self.timesteps = torch.tensor(steps, dtype=torch.int32, device=dev)
        self.rng_state = torch.tensor([int(seed), 0], dtype=torch.int64, device=dev)      # Philox {seed, offset} of the device draws
        self.slot_word = torch.full((1,), -1, dtype=torch.int32, device=dev)              # the slot of the last call, -1: none
        # e where e launched in the last call over all environments, -1 elsewhere (calls on an env_ids list do not write it)
        self.launch_ids = torch.full((self.num_envs,), -1, dtype=torch.int32, device=dev)

    def _operands(self, state):
        proj = state['proj_states']
        if proj.dim() != 3 or proj.shape[0] != self.num_envs or proj.shape[1] < self.n_slots or proj.shape[2] != 13 or proj.stride(2) != 1:
            raise ValueError(f"proj_states must be [{self.num_envs}, >= {self.n_slots}, 13] with unit stride in the last dimension, "
                             f"got {tuple(proj.shape)} strides {tuple(proj.stride())}")
        for k in ('humanoid_root_states', 'rigid_body_pos', 'rigid_body_vel'):
            if state[k].stride(-1) != 1:
                raise ValueError(f"{k} must have unit stride in the last dimension")
        return state['humanoid_root_states'], state['rigid_body_pos'], state['rigid_body_vel'], proj[:, :self.n_slots]

    def _ids(self, env_ids):
        return None if env_ids is None else torch.as_tensor(env_ids, device=self.device).view(-1).to(torch.int32).contiguous()

    def draw(self, n):
        """The draws of one launch of n rows by torch, in the reference's call order and shapes (lines 183-203: rand([n]) for
        theta, distance and height, randn_like of [n, 3], rand_like of [n, 1]): under the same CPU seed, the reference's own
        draws.  -> {'u': f32 [n, 4] = theta, distance, height, speed; 'eps': f32 [n, 3]} on the launcher's device."""
        g = self.generator
        theta, dist, height = (torch.rand([n], generator=g) for _ in range(3))
        eps = torch.randn(n, 3, generator=g)
        speed = torch.rand(n, 1, generator=g)
        u = torch.stack([theta, dist, height, speed[:, 0]], dim=-1)
        return {'u': u.to(self.device), 'eps': eps.to(self.device)}

    def apply(self, state, plan, slot, env_ids=None):
        """Launch projectile `slot` with the draws of ``draw`` for every environment, or for env_ids (row i of the plan
        belongs to env_ids[i]).  ``slot_word`` is written; ``launch_ids`` only without env_ids."""
        ids = self._ids(env_ids)
        self.be.proj_launch(*self._operands(state), slot=int(slot), env_ids=ids, u=plan['u'], eps=plan['eps'], tar_body=self.tar_body,
                            slot_out=self.slot_word, ids_out=self.launch_ids if ids is None else None, **self.params)

    def launch(self, state, slot, env_ids=None):
        """Launch projectile `slot` with device draws, for every environment or for env_ids; one stream position.
        ``slot_word`` is written; ``launch_ids`` only without env_ids."""
        ids = self._ids(env_ids)
        self.be.proj_launch(*self._operands(state), slot=int(slot), env_ids=ids, rng_state=self.rng_state, tar_body=self.tar_body,
                            slot_out=self.slot_word, ids_out=self.launch_ids if ids is None else None, **self.params)

    def update(self, state, progress_buf):
        """_update_proj: the projectile that is due by progress_buf[0], if any, is launched in every environment.  One launch
        whatever the schedule says, one stream position; ``slot_word`` and ``launch_ids`` hold what happened."""
        self.be.proj_launch(*self._operands(state), progress_buf=progress_buf, timesteps=self.timesteps, rng_state=self.rng_state,
                            tar_body=self.tar_body, slot_out=self.slot_word, ids_out=self.launch_ids, **self.params)
