"""The device draws of ``ase_hip_proj_launch``, stated on the host on the stream of tests/ref_rollout.py, and
the schedule of ``HumanoidPerturb._update_proj`` in numpy.  TEST INFRASTRUCTURE ONLY.

Draw j of environment e is element 8 e + j of the stream at the call's (seed, offset):

    j = 0, 1, 2   keep-uniform (24 bits of word 2): theta, distance, height
    j = 3, 4, 5   normal (Box-Muller on words 0 and 1): the noise of the launch direction
    j = 6         keep-uniform: speed
"""
import numpy as np
import torch

from tests import ref_rollout as RR

DRAWS = 7
UNIFORM_J, NORMAL_J = (0, 1, 2, 6), (3, 4, 5)
# the reference's PERTURB_OBJS step counts (env/tasks/humanoid_perturb.py:12-26) and their cumulative sums
PERTURB_STEPS = (60, 7, 10, 35, 2, 2, 3, 2, 2, 3, 2, 60, 300)
PERTURB_TIMESTEPS = np.cumsum(PERTURB_STEPS)


def draw_elems(env_ids):
    e8 = np.uint64(8) * np.asarray(list(env_ids), dtype=np.uint64)
    return e8[:, None] + np.arange(DRAWS, dtype=np.uint64)[None, :]


def device_draws(env_ids, seed, offset, dtype=torch.float32):
    """f32 (or f64 for the normals' arithmetic) [n, 7] in the order j = 0 .. 6.  The uniforms are exact in f32."""
    el = draw_elems(env_ids)
    out = torch.zeros(el.shape, dtype=dtype)
    for j in UNIFORM_J:
        out[:, j] = torch.from_numpy(RR.keep_uniform(RR.philox4x32_10(el[:, j], offset, seed)[2])).to(dtype)
    for j in NORMAL_J:
        out[:, j] = RR.normals(el[:, j], offset, seed, dtype)
    return out


def split(draws):
    """[n, 7] -> (u [n, 4] = theta, distance, height, speed; eps [n, 3]) as ase_hip_proj_launch takes them."""
    return draws[:, list(UNIFORM_J)].contiguous(), draws[:, list(NORMAL_J)].contiguous()


def join(u, eps):
    return torch.cat([u[:, 0:3], eps, u[:, 3:4]], dim=-1)


def due_slot(t, timesteps=PERTURB_TIMESTEPS):
    """The reference's lines 174-179 for a counter value t: the launched object or -1."""
    timesteps = np.asarray(timesteps)
    hit = np.where(timesteps == int(t) % (int(timesteps[-1]) + 1))[0]
    return int(hit[0]) if len(hit) > 0 else -1
