"""Golden vectors of the projectile launches of the perturbation task, recorded from the reference's own
unmodified ``HumanoidPerturb._update_proj``.  TEST INFRASTRUCTURE ONLY (needs the reference tree; isaacgym comes from the
restatement in oracle/rl_games_shim).

    python scripts/make_golden_perturb.py      # writes tests/golden/perturb.pt (tensors, plain lists and numbers only)

The reference's class cannot be constructed without Isaac Gym, but ``_update_proj`` runs on a bare instance
(``object.__new__``) that carries the attributes it reads, with a stub ``gym``.  Each call runs under ``torch.manual_seed``; the
draws are then recovered by repeating its calls under the same seed - rand([n]) x 3, randn(n, 3), rand(n, 1) - and the
restatement tests/emu_perturb.py on those draws must reproduce the reference's f32 result bit for bit.

What the file carries and why:
  inputs      n = 32 environments, 2 bodies, seeded root states and body positions / velocities; the packed root tensor
              [n * A, 13] before a chain is an arithmetic pattern around the root states (tests/emu_perturb.py packed_before),
              not stored.
  cases       A = 14 and 15 actors per environment (13 projectiles behind one and two other actors).  Per case a chain of five
              calls on ONE tensor at progress 59 (not due), 60 (slot 0), 77 (slot 2), 488 (slot 12) and 489 + 67 (the wrap:
              slot 1).  Every call reads only the humanoid's rows and writes a slot of its own, so the tensor after the chain
              holds every call's result: it is stored WHOLE, untouched actors and slots are part of the record.  The call at
              59 is asserted here to change nothing and to draw nothing.
  draws       per due call [n, 7] in the order of the device draws: theta, distance, height, noise x 3, speed
              (tests/ref_perturb.py split gives the entry's u [n, 4] and eps [n, 3]).
  e_ref       per due call and group (position, velocity) max |reference f32 - f64 restatement|: the device tests allow
              2 e_ref + 2^-23 max |ref| + 1e-7 against f64.  Asserted here to be at most 16 * 2^-24 * max |group| - a handful
              of f32 roundings - so that a bad draw cannot loosen the tests.
  conditions  seeds are walked from 0 until every uniform lies strictly inside (0, 1).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('ASE_REFERENCE', '/root/reference/ase')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'rl_games_shim'))
sys.path.insert(0, REFERENCE)

from env.tasks import humanoid_perturb as HP                  # noqa: E402  (reference code)

from tests import emu_perturb as E                            # noqa: E402
from tests import ref_perturb as RP                           # noqa: E402

N, BODIES, TAR_BODY = 32, 2, 1
ACTORS = (14, 15)
PROGRESS = (59, 60, 77, 488, 489 + 67)
ROUNDINGS = 16                                                # e_ref cap: this many f32 roundings of the group's largest output


class _Gym:
    """The one simulator call of _update_proj: counted, nothing else."""

    def __init__(self):
        self.sets = 0

    def set_actor_root_state_tensor_indexed(self, sim, states, ids, n):
        self.sets += 1


def draw_inputs():
    g = torch.Generator().manual_seed(20271)
    root = torch.randn(N, 13, generator=g)
    root[:, 0:3] = root[:, 0:3] * torch.tensor([3.0, 3.0, 0.1]) + torch.tensor([0.0, 0.0, 0.9])
    root[:, 3:7] = root[:, 3:7] / root[:, 3:7].norm(dim=-1, keepdim=True)
    body_pos = root[:, None, 0:3] + 0.3 * torch.randn(N, BODIES, 3, generator=g)
    body_vel = 2.0 * torch.randn(N, BODIES, 3, generator=g)
    return root, body_pos.contiguous(), body_vel.contiguous()


def bare(G, packed, actors, progress):
    """An instance of the reference's class without its constructor, carrying what _update_proj reads."""
    o = object.__new__(HP.HumanoidPerturb)
    HP.HumanoidPerturb._calc_perturb_times(o)
    o._proj_dist_min, o._proj_dist_max, o._proj_h_min, o._proj_h_max = 4, 5, 0.25, 2           # humanoid_perturb.py:37-44
    o._proj_speed_min, o._proj_speed_max = 30, 40
    o.num_envs, o.num_bodies, o.gym, o.sim = N, BODIES, _Gym(), None
    o.progress_buf = torch.full((N,), progress, dtype=torch.int64)
    o._root_states = packed
    o._humanoid_root_states, o._proj_states = E.views(G, packed, actors)
    o._rigid_body_pos, o._rigid_body_vel = G['body_pos'], G['body_vel']
    o._proj_actor_ids = torch.zeros(N * len(HP.PERTURB_OBJS), dtype=torch.int32)
    return o


def recover_draws(seed):
    """The same calls as _update_proj under the same seed -> (u [n, 4], eps [n, 3])."""
    torch.manual_seed(seed)
    theta, dist, height = torch.rand([N]), torch.rand([N]), torch.rand([N])
    eps = torch.randn(N, 3)
    speed = torch.rand(N, 1)
    return torch.stack([theta, dist, height, speed[:, 0]], dim=-1), eps


def build():
    root, body_pos, body_vel = draw_inputs()
    steps = [int(o[1]) for o in HP.PERTURB_OBJS]
    assert tuple(steps) == RP.PERTURB_STEPS
    G = {'num_envs': N, 'num_bodies': BODIES, 'tar_body': TAR_BODY, 'steps': steps, 'timesteps': np.cumsum(steps).tolist(),
         'params': dict(E.DEFAULTS), 'root_states': root, 'body_pos': body_pos, 'body_vel': body_vel, 'roundings': ROUNDINGS,
         'cases': {}}
    seed = 0
    for A in ACTORS:
        packed = E.packed_before(G, A)
        before = packed.clone()
        chain = []
        for progress in PROGRESS:
            want = RP.due_slot(progress)
            prev = packed.clone()
            while True:
                o = bare(G, packed, A, progress)
                assert o._perturb_timesteps.tolist() == G['timesteps']
                torch.manual_seed(seed)
                state = torch.get_rng_state()
                HP.HumanoidPerturb._update_proj(o)
                if want < 0:
                    assert torch.equal(packed, prev) and o.gym.sets == 0 and torch.equal(torch.get_rng_state(), state)
                    chain.append({'progress': progress, 'slot': -1, 'seed': seed, 'draws': None, 'e_ref': None})
                    break
                assert o.gym.sets == 1
                u, eps = recover_draws(seed)
                seed += 1
                if bool(((u > 0) & (u < 1)).all()):
                    chain.append({'progress': progress, 'slot': want, 'seed': seed - 1, 'draws': RP.join(u, eps)})
                    break
                packed.copy_(prev)
        case = {'actors': A, 'chain': chain, 'after': packed.clone()}
        # the restatement on the recovered draws: f32 bit for bit the reference, f64 the yardstick
        f32, f64 = E.replay(G, case, torch.float32), E.replay(G, case, torch.float64)
        assert torch.equal(f32, packed), f'A = {A}: the f32 restatement is not bitwise the reference'
        _, proj = E.views(G, packed, A)
        _, proj64 = E.views(G, f64, A)
        _, proj0 = E.views(G, before, A)
        written = [st['slot'] for st in chain if st['slot'] >= 0]
        others = [k for k in range(len(steps)) if k not in written]
        assert torch.equal(proj[:, others], proj0[:, others]) and torch.equal(packed.view(N, A, 13)[:, :A - len(steps)],
                                                                               before.view(N, A, 13)[:, :A - len(steps)])
        for st in chain:
            if st['slot'] < 0:
                continue
            row, row64 = proj[:, st['slot']], proj64[:, st['slot']]
            assert torch.equal(row[:, E.CONSTANT_COLS], E.CONSTANT.expand(N, 7))
            st['e_ref'] = {}
            for g, cols in E.GROUPS.items():
                e = float((row[:, cols].double() - row64[:, cols]).abs().max())
                cap = ROUNDINGS * 2.0 ** -24 * float(row[:, cols].abs().max())
                assert e <= cap, f'A = {A} progress {st["progress"]} {g}: the reference itself loses {e:.3g} in f32 (cap {cap:.3g})'
                st['e_ref'][g] = e
                print(f'A {A} progress {st["progress"]:4d} slot {st["slot"]:2d} seed {st["seed"]:3d} {g}: |ref - f64| {e:.3g} (cap {cap:.3g})')
        G['cases'][f'A{A}'] = case
    return G


def main():
    G = build()
    path = os.path.join(ROOT, 'tests', 'golden', 'perturb.pt')
    torch.save(G, path)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 64 * 1024, 'two packed tensors and the draws'


if __name__ == '__main__':
    main()
