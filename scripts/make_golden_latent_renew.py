"""Golden vectors of the ASE agent's latent renewals, recorded from the reference's own unmodified methods.
TEST INFRASTRUCTURE ONLY (needs the reference tree; rl_games and isaacgym come from the restatement in oracle/rl_games_shim).

    python scripts/make_golden_latent_renew.py      # writes tests/golden/latent_renew.pt (tensors, plain lists and numbers only)

The reference's ``ASEAgent`` cannot be constructed without Isaac Gym and rl_games' runner, but ``env_reset`` and
``_update_latents`` run on a bare instance (``object.__new__``) that carries the attributes they read: ``_ase_latents``,
``_latent_reset_steps``, ``_latent_steps_min / max``, ``ppo_device``, a ``vec_env.env.task`` stub (``progress_buf``,
``num_envs``, ``viewer = None``) and a ``model.a2c_network`` stub whose ``sample_latents`` is the reference's function from
``ASEBuilder.Network``, bound to a stub with an ``_enc`` parameter and ``_ase_latent_shape``.  Each runs under
``torch.manual_seed``; the draws are then recovered by repeating the same ``torch.normal`` / ``torch.randint_like`` calls under
the same seed, and the restatement tests/emu_latent_renew.py on those draws must reproduce the reference's f32 result.

What the file carries and why:
  inputs      N = 32 environments, dim = 64, steps in [1, 150) (latent_steps_min / max of the reference's yaml); the latents
              before a scenario are an arithmetic pattern (tests/emu_latent_renew.py prefill), not stored.
  scenarios   reset_ids (env_reset on 20 distinct shuffled ids), reset_all (env_reset()), update (_update_latents on a seeded
              progress_buf / reset_steps).  Per scenario the ids, the draws (eps [n, dim], steps int32 [n]) and the reference's
              outputs as WHOLE tensors, so that untouched rows are part of the record.
  e_ref       per scenario max |reference f32 - f64 restatement| of the normalisation on the recorded eps: the allowance of
              the device tests (2 e_ref + 1e-7 against f64).  Asserted here to be at most 16 * 2^-24 - a handful of f32
              roundings of 1.0, the largest possible output - so that a bad draw cannot loosen the tests.
  conditions  seeds are walked from 0 until: no eps row has a norm below 1 (the 1e-12 floor is far away); update has at least
              6 due and 6 not-due rows.  One update row is set to reset_steps == progress_buf, the <= edge, and one to
              reset_steps == progress_buf + 1, just not due.
"""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('ASE_REFERENCE', '/root/reference/ase')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'rl_games_shim'))
sys.path.insert(0, REFERENCE)

from learning.ase_agent import ASEAgent                       # noqa: E402  (reference code)
from learning.ase_network_builder import ASEBuilder           # noqa: E402

from tests import emu_latent_renew as E                       # noqa: E402

N, DIM, N_IDS = 32, 64, 20
STEPS_LOW, STEPS_HIGH = 1, 150                                # latent_steps_min / max, data/cfg/train/rlg/ase_humanoid.yaml
MIN_GROUP, ROUNDINGS = 6, 16
EDGE_ROW, BELOW_ROW = 3, 4                                    # update: reset_steps == progress_buf / == progress_buf + 1


def yaml_steps():
    import yaml
    with open(os.path.join(REFERENCE, 'data', 'cfg', 'train', 'rlg', 'ase_humanoid.yaml')) as f:
        c = yaml.safe_load(f)['params']['config']
    return c['latent_steps_min'], c['latent_steps_max']


def bare(latents, reset_steps, progress_buf):
    """An instance of the reference's agent without its constructor, carrying what the two methods read."""
    net = types.SimpleNamespace(_enc=torch.nn.Linear(1, 1), _ase_latent_shape=(DIM,))
    net.sample_latents = types.MethodType(ASEBuilder.Network.sample_latents, net)
    task = types.SimpleNamespace(progress_buf=progress_buf, num_envs=N, viewer=None)
    o = object.__new__(ASEAgent)
    o.ppo_device = 'cpu'
    o._ase_latents, o._latent_reset_steps = latents, reset_steps
    o._latent_steps_min, o._latent_steps_max = STEPS_LOW, STEPS_HIGH
    o.model = types.SimpleNamespace(a2c_network=net)
    o.vec_env = types.SimpleNamespace(env=types.SimpleNamespace(task=task), reset=lambda env_ids=None: torch.zeros(N, 1))
    o.obs_to_tensors = lambda obs: {'obs': obs}               # CommonAgent.env_reset's own part: no latents involved
    return o


def recover_draws(n, seed):
    """The same torch.normal / torch.randint_like calls as the reference's methods, under the same seed."""
    torch.manual_seed(seed)
    eps = torch.normal(torch.zeros([n, DIM]))
    steps = torch.randint_like(torch.zeros(n, dtype=torch.int32), low=STEPS_LOW, high=STEPS_HIGH)
    return eps, steps


def update_inputs(seed):
    g = torch.Generator().manual_seed(4000 + seed)
    progress = torch.randint(0, 300, (N,), generator=g)                                   # long, as the reference's
    reset_steps = (progress + torch.randint(-40, 40, (N,), generator=g)).to(torch.int32)
    reset_steps[EDGE_ROW] = int(progress[EDGE_ROW])
    reset_steps[BELOW_ROW] = int(progress[BELOW_ROW]) + 1
    return progress, reset_steps


def run_scenario(G, name, seed):
    sc = {'seed': seed}
    if name == 'update':
        sc['progress_buf'], sc['reset_steps0'] = update_inputs(seed)
    G['scenarios'][name] = sc
    latents, reset_steps, progress = E.prefill(G, name)
    o = bare(latents, reset_steps, progress)
    torch.manual_seed(seed)
    if name == 'reset_ids':
        ids = torch.randperm(N, generator=torch.Generator().manual_seed(20269))[:N_IDS]
        ASEAgent.env_reset(o, ids)
    elif name == 'reset_all':
        ids = torch.arange(N)
        ASEAgent.env_reset(o)
    else:
        ids = (sc['reset_steps0'] <= progress).nonzero().flatten()
        ASEAgent._update_latents(o)
    sc['env_ids'] = ids.tolist()
    sc['eps'], sc['steps'] = recover_draws(len(ids), seed)
    sc['latents'], sc['reset_steps'] = latents.clone(), reset_steps.clone()
    return sc


def acceptable(G, name):
    sc = G['scenarios'][name]
    ok = float(sc['eps'].norm(dim=-1).min()) >= 1.0
    if name == 'update':
        due = len(sc['env_ids'])
        ok = ok and due >= MIN_GROUP and N - due >= MIN_GROUP
    return ok


def build():
    assert yaml_steps() == (STEPS_LOW, STEPS_HIGH)
    G = {'num_envs': N, 'dim': DIM, 'steps_low': STEPS_LOW, 'steps_high': STEPS_HIGH, 'roundings': ROUNDINGS,
         'edge_row': EDGE_ROW, 'below_row': BELOW_ROW, 'scenarios': {}}
    for name in E.SCENARIOS:
        for seed in range(200):
            sc = run_scenario(G, name, seed)
            if acceptable(G, name):
                break
        else:
            raise AssertionError(f'{name}: no seed below 200 meets the conditions')
        ids = sc['env_ids']
        others = [e for e in range(N) if e not in ids]
        lat0, steps0, progress = E.prefill(G, name)
        assert torch.equal(sc['latents'][others], lat0[others]) and torch.equal(sc['reset_steps'][others], steps0[others])
        assert bool(((sc['steps'] >= STEPS_LOW) & (sc['steps'] < STEPS_HIGH)).all()) and sc['steps'].dtype == torch.int32
        if name == 'update':
            assert EDGE_ROW in ids and BELOW_ROW not in ids and torch.equal(progress, sc['progress_buf'])
        # the pin of the restatement to the reference in f32, whole tensors: bitwise
        l32, s32 = E.expected(G, name, torch.float32)
        assert torch.equal(l32, sc['latents']) and torch.equal(s32, sc['reset_steps']), name
        l64, s64 = E.expected(G, name, torch.float64)
        assert torch.equal(s64, sc['reset_steps'])
        sc['e_ref'] = float((sc['latents'][ids].double() - l64[ids]).abs().max())
        assert sc['e_ref'] <= ROUNDINGS * 2.0 ** -24, f'{name}: the reference itself loses {sc["e_ref"]:.3g} in f32'
        print(f'{name:10s} seed {seed:3d}  rows {len(ids):2d}  |ref - f64| {sc["e_ref"]:.3g} (cap {ROUNDINGS * 2.0 ** -24:.3g})')
    return G


def main():
    G = build()
    path = os.path.join(ROOT, 'tests', 'golden', 'latent_renew.pt')
    torch.save(G, path)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 64 * 1024, 'a few tens of KB are enough'


if __name__ == '__main__':
    main()
