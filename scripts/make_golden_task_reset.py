"""Golden vectors of the target resets of the four tasks, recorded from the reference's own unmodified
methods.  TEST INFRASTRUCTURE ONLY (needs the reference tree; isaacgym comes from the restatement in oracle/rl_games_shim).

    python scripts/make_golden_task_reset.py      # writes tests/golden/task_reset.pt (tensors, plain lists and numbers only)

The reference's task classes cannot be constructed without Isaac Gym, but ``_reset_task`` / ``_reset_target`` run on a bare
instance (``object.__new__``) that carries the attributes they read.  Each runs under ``torch.manual_seed``; the draws are then
recovered by repeating the same ``torch.rand`` / ``torch.randint`` calls under the same seed, and the restatement
tests/emu_task_reset.py on those draws must reproduce the reference's f32 result.

What the file carries and why:
  inputs      N = 32 environments, 20 distinct shuffled env_ids, a seeded progress_buf and seeded root states; the targets
              before a reset are an arithmetic pattern (tests/emu_task_reset.py prefill), not stored.
  defaults    the reset parameters of the reference's task yaml files (the strike task's are literals of its constructor):
              what HumanoidTensors takes when the caller gives none.
  scenarios   heading, heading_fixed (enable_rand_heading off), location, reach, strike.  Per scenario the parameters, the
              draws (u [n, U] in the order of the torch.rand calls, steps) and the reference's f32 outputs as WHOLE tensors, so
              that untouched rows are part of the record.
  f64         the restatement on the recorded f32 draws cast up, recomputed by the tests.
  e_ref       per scenario and output group max |reference f32 - f64|: the allowance of the device tests (2 e_ref + 1e-7
              against f64).  Asserted here to be at most 16 * 2^-24 * max |output of the group| - a handful of f32 roundings -
              so that a bad draw cannot loosen the tests.
  conditions  seeds are walked from 0 until: every u lies strictly inside (0, 1); strike has at least 4 near and 4 far rows
              and no u0 within 1e-3 of near_prob (the near test is then the same in every precision).
"""
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('ASE_REFERENCE', '/root/reference/ase')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'rl_games_shim'))
sys.path.insert(0, REFERENCE)

from env.tasks.humanoid_heading import HumanoidHeading        # noqa: E402  (reference code)
from env.tasks.humanoid_location import HumanoidLocation      # noqa: E402
from env.tasks.humanoid_reach import HumanoidReach            # noqa: E402
from env.tasks.humanoid_strike import HumanoidStrike          # noqa: E402

from tests import emu_task_reset as E                         # noqa: E402

N, N_IDS = 32, 20
MARGIN, MIN_GROUP = 1e-3, 4
ROUNDINGS = 16                                                # e_ref cap: this many f32 roundings of the group's largest output
YAML_KEYS = {'tarSpeedMin': 'tar_speed_min', 'tarSpeedMax': 'tar_speed_max', 'headingChangeStepsMin': 'heading_change_steps_min',
             'headingChangeStepsMax': 'heading_change_steps_max', 'enableRandHeading': 'enable_rand_heading',
             'tarChangeStepsMin': 'tar_change_steps_min', 'tarChangeStepsMax': 'tar_change_steps_max', 'tarDistMax': 'tar_dist_max',
             'tarHeightMin': 'tar_height_min', 'tarHeightMax': 'tar_height_max'}


def defaults():
    out = {}
    for task in ('heading', 'location', 'reach'):
        with open(os.path.join(REFERENCE, 'data', 'cfg', f'humanoid_sword_shield_{task}.yaml')) as f:
            env = yaml.safe_load(f)['env']
        out[task] = {YAML_KEYS[k]: v for k, v in env.items() if k in YAML_KEYS}
    out['strike'] = dict(tar_dist_min=0.5, tar_dist_max=10.0, near_dist=1.5, near_prob=0.5)      # humanoid_strike.py:19-22
    return out


def draw_inputs():
    g = torch.Generator().manual_seed(20268)
    root = torch.randn(N, 13, generator=g)
    root[:, 0:3] = root[:, 0:3] * torch.tensor([3.0, 3.0, 0.1]) + torch.tensor([0.0, 0.0, 0.9])
    root[:, 3:7] = root[:, 3:7] / root[:, 3:7].norm(dim=-1, keepdim=True)
    progress = torch.randint(0, 300, (N,), generator=g)
    env_ids = torch.randperm(N, generator=g)[:N_IDS]
    return root, progress, env_ids.tolist()


def bare(G, task, params):
    """An instance of the reference's class without its constructor, carrying what the reset method reads."""
    cls = {'heading': HumanoidHeading, 'location': HumanoidLocation, 'reach': HumanoidReach, 'strike': HumanoidStrike}[task]
    s, progress, change = E.prefill(G, task)
    o = object.__new__(cls)
    o.device, o.progress_buf = 'cpu', progress
    o._humanoid_root_states = s['humanoid_root_states']
    for k, v in params.items():
        setattr(o, '_' + k, v)
    if task == 'heading':
        o._tar_dir, o._tar_facing_dir, o._tar_speed, o._heading_change_steps = s['tar_dir'], s['tar_facing_dir'], s['tar_speed'], change
    elif task == 'strike':
        o._target_states = s['target_states']
    else:
        o._tar_pos, o._tar_change_steps = s['tar_pos'], change
    return cls, o, s, change


def recover_draws(task, params, n, seed):
    """The same torch.rand / torch.randint calls as the reference's method, under the same seed -> (u [n, U], steps)."""
    torch.manual_seed(seed)
    if task == 'heading':
        angles = [torch.rand(n), torch.rand(n)] if params['enable_rand_heading'] else [torch.zeros(n), torch.zeros(n)]
        u = torch.stack(angles + [torch.rand(n)], dim=-1)
        return u, torch.randint(low=params['heading_change_steps_min'], high=params['heading_change_steps_max'], size=(n,), dtype=torch.int64)
    if task == 'strike':
        return torch.stack([torch.rand([n]) for _ in range(4)], dim=-1), None
    u = torch.rand([n, 2 if task == 'location' else 3])
    return u, torch.randint(low=params['tar_change_steps_min'], high=params['tar_change_steps_max'], size=(n,), dtype=torch.int64)


def run_scenario(G, task, params, seed):
    cls, o, s, change = bare(G, task, params)
    env_ids = torch.tensor(G['env_ids'], dtype=torch.long)
    torch.manual_seed(seed)
    if task == 'strike':
        cls._reset_target(o, env_ids)
    else:
        cls._reset_task(o, env_ids)
    u, steps = recover_draws(task, params, len(env_ids), seed)
    f32 = {k: v.clone() for k, v in E.outputs(task, s, change).items()}
    return {'task': task, 'seed': seed, 'params': dict(params), 'u': u, 'steps': steps, 'f32': f32}


def acceptable(sc):
    u, p = sc['u'], sc['params']
    drawn = u if p.get('enable_rand_heading', True) else u[:, 2:]
    ok = bool(((drawn > 0) & (drawn < 1)).all())
    if sc['task'] == 'strike':
        near = u[:, 0] < p['near_prob']
        ok = ok and int(near.sum()) >= MIN_GROUP and int((~near).sum()) >= MIN_GROUP
        ok = ok and float((u[:, 0].double() - p['near_prob']).abs().min()) > MARGIN
    return ok


def errors(G, sc):
    """(per float group max |reference f32 - f64| on the reset rows, the same against the f32 restatement, the cap)."""
    ids = G['env_ids']
    f64, f32 = E.expected(G, sc, torch.float64), E.expected(G, sc, torch.float32)
    e_ref, pin, cap = {}, {}, {}
    for g in E.FLOAT_GROUPS[sc['task']]:
        ref = sc['f32'][g]
        e_ref[g] = float((ref[ids].double() - f64[g][ids]).abs().max())
        pin[g] = float((ref - f32[g]).abs().max())
        cap[g] = ROUNDINGS * 2.0 ** -24 * float(ref[ids].abs().max())
    for g in set(sc['f32']) - set(E.FLOAT_GROUPS[sc['task']]):      # change steps, strike's constant columns: exact in every run
        assert torch.equal(sc['f32'][g], f32[g]) and torch.equal(sc['f32'][g], f64[g].to(sc['f32'][g].dtype)), g
    return e_ref, pin, cap


def build():
    root, progress, env_ids = draw_inputs()
    D = defaults()
    G = {'num_envs': N, 'env_ids': env_ids, 'root_states': root, 'progress_buf': progress, 'margin': MARGIN, 'roundings': ROUNDINGS,
         'defaults': D, 'scenarios': {}}
    specs = [('heading', 'heading', D['heading']), ('heading_fixed', 'heading', dict(D['heading'], enable_rand_heading=False)),
             ('location', 'location', D['location']), ('reach', 'reach', D['reach']), ('strike', 'strike', D['strike'])]
    for name, task, params in specs:
        for seed in range(200):
            sc = run_scenario(G, task, params, seed)
            if acceptable(sc):
                break
        else:
            raise AssertionError(f'{name}: no seed below 200 meets the conditions')
        e_ref, pin, cap = errors(G, sc)
        others = [e for e in range(N) if e not in env_ids]
        state0, _, change0 = E.prefill(G, task)
        before = E.outputs(task, state0, change0)
        for g, v in sc['f32'].items():
            assert torch.equal(v[others], before[g][others]), f'{name}: a row of {g} outside env_ids changed'
        for g in e_ref:
            # the pin of the restatement to the reference in f32: a few ulp of the group's largest output at the most
            assert pin[g] <= 4 * 2.0 ** -24 * max(1.0, float(sc['f32'][g][env_ids].abs().max())), (name, g, pin[g])
            assert e_ref[g] <= cap[g], f'{name} {g}: the reference itself loses {e_ref[g]:.3g} in f32 (cap {cap[g]:.3g})'
        sc['e_ref'], sc['bitwise'] = e_ref, {g: pin[g] == 0.0 for g in pin}
        G['scenarios'][name] = sc
        print(f'{name:14s} seed {seed:3d}  ' + '  '.join(f'{g}: |ref - f64| {e_ref[g]:.3g} (cap {cap[g]:.3g}) |emu f32 - ref| {pin[g]:.3g}'
                                                        for g in e_ref))
    return G


def main():
    G = build()
    path = os.path.join(ROOT, 'tests', 'golden', 'task_reset.pt')
    torch.save(G, path)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 64 * 1024, 'a few KB are enough'


if __name__ == '__main__':
    main()
