"""Plain-torch restatement of ``HipBackend.task_reset`` with the same signature, the host statement of its
device draws, and the helpers of the fixture tests/golden/task_reset.pt (scripts/make_golden_task_reset.py).
TEST INFRASTRUCTURE ONLY: the CPU stand-in for the backend in the host tests and the f64 leg of the fixture.

Written from the contract in include/ase_hip.h, following env/tasks/humanoid_heading.py:147-174, humanoid_location.py:107-125,
humanoid_reach.py:111-130 and humanoid_strike.py:108-128 of the reference.  The arithmetic runs in the dtype of the target
tensors: f32 repeats the reference's operations (its Python scalars enter a product as f32 roundings of the f64 constants),
f64 is the yardstick on the same f32 draws cast up."""
import math
import os

import numpy as np
import torch

from ase_amd import lib as L
from tests import ref_rollout as RR

TASKS = ('heading', 'location', 'reach', 'strike')
KIND = {'heading': L.TASK_HEADING, 'location': L.TASK_LOCATION, 'reach': L.TASK_REACH, 'strike': L.TASK_STRIKE}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---- the device draws, stated on the host ------------------------------------------------------------------------------------
def reduce_steps(word, low, high):
    """The change steps of a 32-bit word: low + floor(word * (high - low) / 2^32), exact integers, in [low, high)."""
    return int(low) + ((int(word) * (int(high) - int(low))) >> 32)


def device_draws(kind, env_ids, seed, offset, low=0, high=1):
    """(u f32 [n, U], steps int64 [n]) as ase_hip_task_reset draws them for the environments env_ids: uniform j of
    environment e is the keep-uniform (24 bits of word 2) of element 4 e + j of the stream at (seed, offset), the change steps
    come from word 0 of element 4 e + 3."""
    e4 = np.uint64(4) * np.asarray(list(env_ids), dtype=np.uint64)
    U = L.TASK_RESET_DRAWS[kind]
    u = np.stack([RR.keep_uniform(RR.philox4x32_10(e4 + np.uint64(j), offset, seed)[2]) for j in range(U)], axis=-1)
    w0 = RR.philox4x32_10(e4 + np.uint64(3), offset, seed)[0]
    steps = torch.tensor([reduce_steps(w, low, high) for w in w0], dtype=torch.int64)
    return torch.from_numpy(u.reshape(len(e4), U)), steps


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _quat_from_angle_z(angle):
    """isaacgym.torch_utils.quat_from_angle_axis about z: {axis / |axis| sin(angle / 2), cos(angle / 2)}, normalised."""
    theta = (angle / 2).unsqueeze(-1)
    axis = torch.tensor([0.0, 0.0, 1.0], dtype=angle.dtype)
    xyz = axis / axis.norm(p=2, dim=-1).clamp(min=1e-9).unsqueeze(-1) * theta.sin()
    q = torch.cat([xyz, theta.cos()], dim=-1)
    return q / q.norm(p=2, dim=-1).clamp(min=1e-9).unsqueeze(-1)


class EmuTaskReset:
    name = "emu-task-reset"
    device = torch.device('cpu')

    def task_reset(self, kind, progress_buf=None, change_steps=None, root_states=None, tar_a=None, tar_b=None, tar_speed=None,
                   tar_states=None, env_ids=None, u=None, steps=None, rng_state=None, advance=True, steps_low=0, steps_high=0,
                   tar_speed_min=0.0, tar_speed_max=0.0, tar_dist_min=0.0, tar_dist_max=0.0, tar_height_min=0.0, tar_height_max=0.0,
                   near_dist=0.0, near_prob=0.0, enable_rand_heading=True):
        strike = kind == L.TASK_STRIKE
        assert (u is None) != (rng_state is None), 'exactly one draw source'
        assert env_ids is not None or (not strike and u is None), 'due mode: not for strike, device draws only'
        out = tar_states if strike else tar_a
        n, dt = out.shape[0], out.dtype
        if env_ids is None:
            ids = (progress_buf >= change_steps).nonzero().flatten()
        else:
            ids = env_ids.long()
            keep = (ids >= 0) & (ids < n)                         # ids outside the buffers are skipped
            ids = ids[keep]
            if u is not None:
                u, steps = u[keep], None if steps is None else steps[keep]
        if u is None:
            seed, offset = int(rng_state[0]), int(rng_state[1])
            u, steps = device_draws(kind, ids.tolist(), seed, offset, steps_low, steps_high)
            if strike:
                steps = None
            if advance:
                rng_state[1] += 1
        if ids.numel() == 0:
            return
        u = u.to(dt)                                              # the draws are f32 values in both runs
        c = lambda x: torch.tensor(x, dtype=torch.float32).to(dt) if dt == torch.float32 else torch.tensor(x, dtype=dt)
        two_pi, pi = c(2 * math.pi), c(math.pi)
        if kind == L.TASK_HEADING:
            zeros = torch.zeros(ids.numel(), dtype=dt)
            theta = two_pi * u[:, 0] - pi if enable_rand_heading else zeros
            face = two_pi * u[:, 1] - pi if enable_rand_heading else zeros
            tar_a[ids] = torch.stack([torch.cos(theta), torch.sin(theta)], dim=-1)
            tar_b[ids] = torch.stack([torch.cos(face), torch.sin(face)], dim=-1)
            tar_speed[ids] = c(tar_speed_max - tar_speed_min) * u[:, 2] + c(tar_speed_min)
        elif kind == L.TASK_LOCATION:
            tar_a[ids] = root_states[ids, 0:2] + c(tar_dist_max) * (2.0 * u[:, 0:2] - 1.0)
        elif kind == L.TASK_REACH:
            pos = u.clone()
            pos[:, 0:2] = c(tar_dist_max) * (2.0 * pos[:, 0:2] - 1.0)
            pos[:, 2] = c(tar_height_max - tar_height_min) * pos[:, 2] + c(tar_height_min)
            tar_a[ids] = pos
        else:
            near = u[:, 0] < c(near_prob)
            dist_max = torch.where(near, c(near_dist), c(tar_dist_max))
            dist = (dist_max - c(tar_dist_min)) * u[:, 1] + c(tar_dist_min)
            theta = two_pi * u[:, 2]
            tar_states[ids, 0] = dist * torch.cos(theta) + root_states[ids, 0]
            tar_states[ids, 1] = dist * torch.sin(theta) + root_states[ids, 1]
            tar_states[ids, 2] = c(0.9)
            tar_states[ids, 3:7] = _quat_from_angle_z(two_pi * u[:, 3])
            tar_states[ids, 7:13] = 0.0
        if not strike:
            change_steps[ids] = progress_buf[ids] + steps


# ---- the fixture tests/golden/task_reset.pt (scripts/make_golden_task_reset.py) ------------------------------------------------
def load_fixture():
    return torch.load(os.path.join(GOLDEN, 'task_reset.pt'), weights_only=False)


def pattern(*shape):
    """The targets before a reset: an arithmetic pattern, so that untouched rows and columns are detectable."""
    n = int(np.prod(shape))
    return ((torch.arange(n) * 7919) % 2003).to(torch.float32).view(*shape) / 100.0 - 50.0


def prefill(G, task, dtype=torch.float32, device='cpu'):
    """The state before a scenario's reset under the names HumanoidTensors reads -> (state, progress_buf, change_steps)."""
    N = G['num_envs']
    s = {'humanoid_root_states': G['root_states'].clone()}
    if task == 'heading':
        s.update(tar_dir=pattern(N, 2), tar_facing_dir=pattern(N, 2) + 1.0, tar_speed=pattern(N) + 2.0)
    elif task == 'location':
        s.update(tar_pos=pattern(N, 2))
    elif task == 'reach':
        s.update(tar_pos=pattern(N, 3))
    else:
        s.update(target_states=pattern(N, 13))
    s = {k: v.to(dtype).contiguous().to(device) for k, v in s.items()}
    change = None if task == 'strike' else (torch.arange(N, dtype=torch.int64) * 13 + 5).to(device)
    return s, G['progress_buf'].clone().to(device), change


def outputs(task, state, change_steps):
    """The tensors a scenario writes, by output group.  FLOAT_GROUPS are held to the allowance, every other group is exact."""
    s = state
    if task == 'heading':
        return {'tar_dir': s['tar_dir'], 'tar_facing_dir': s['tar_facing_dir'], 'tar_speed': s['tar_speed'], 'change_steps': change_steps}
    if task == 'strike':
        ts = s['target_states']
        return {'target_pos': ts[:, 0:2], 'target_rot': ts[:, 3:7], 'target_rest': ts[:, [2, 7, 8, 9, 10, 11, 12]]}
    return {'tar_pos': s['tar_pos'], 'change_steps': change_steps}


FLOAT_GROUPS = {'heading': ('tar_dir', 'tar_facing_dir', 'tar_speed'), 'location': ('tar_pos',), 'reach': ('tar_pos',),
                'strike': ('target_pos', 'target_rot')}


def operands(task, state, progress_buf, change_steps):
    """Keyword operands of task_reset for a task on a state of prefill()."""
    s = state
    kw = {} if task == 'strike' else dict(progress_buf=progress_buf, change_steps=change_steps)
    if task == 'heading':
        kw.update(tar_a=s['tar_dir'], tar_b=s['tar_facing_dir'], tar_speed=s['tar_speed'])
    elif task == 'location':
        kw.update(root_states=s['humanoid_root_states'], tar_a=s['tar_pos'])
    elif task == 'reach':
        kw.update(tar_a=s['tar_pos'])
    else:
        kw.update(root_states=s['humanoid_root_states'], tar_states=s['target_states'])
    return kw


def params_of(sc):
    """A scenario's parameters as the keyword arguments of task_reset."""
    p = dict(sc['params'])
    for prefix in ('heading', 'tar'):
        if prefix + '_change_steps_min' in p:
            p['steps_low'], p['steps_high'] = p.pop(prefix + '_change_steps_min'), p.pop(prefix + '_change_steps_max')
    return p


def plan_of(G, sc, device='cpu'):
    return {'env_ids': torch.tensor(G['env_ids'], dtype=torch.int32, device=device), 'u': sc['u'].to(device),
            'steps': None if sc['steps'] is None else sc['steps'].to(device)}


def expected(G, sc, dtype=torch.float64):
    """A scenario's result by the restatement on the recorded f32 draws -> the output groups (floats in dtype)."""
    task = sc['task']
    s, progress, change = prefill(G, task, dtype)
    p = plan_of(G, sc)
    EmuTaskReset().task_reset(KIND[task], env_ids=p['env_ids'], u=p['u'], steps=p['steps'], **operands(task, s, progress, change),
                              **params_of(sc))
    return outputs(task, s, change)


def allowance(G, scenario, group):
    """The bar of the device tests: max |x - f64| <= 2 e_ref + 1e-7, e_ref = what the reference's own f32 run loses against the
    f64 result (stored by the generator per scenario and output group)."""
    return 2.0 * G['scenarios'][scenario]['e_ref'][group] + 1e-7
