"""The HRL inner loop's glue without a GPU: the CPU stand-in (tests/emu_hrl_step.py) on every case and bar of
tests/test_gpu_hrl_step.py, the fixture conditions those cases promise, five wrong restatements that each miss a bar, every
refusal of the three C entries (no launch: each call also carries n = 0, which the last check refuses), and ``HRLAgent`` /
``HRLPlayer`` with ``device_llc_step`` on the stand-in against the reference's golden step and the default path."""
import ctypes
import os

import pytest
import torch

import tests.test_boundary_emu as T
from ase_amd import lib as L
from ase_amd.learning import agents, players
from ase_amd.synthetic import EnvSpec, SyntheticVecEnv
from tests import ref_hrl_step as R
from tests.emu_hrl_step import EmuHrlStep
from tests.helpers import BUILDERS

DEV = 'cpu'


@pytest.fixture(scope='module')
def be():
    return EmuHrlStep()


# ---- the stand-in on the GPU file's cases --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', R.LATENT_DIM)
@pytest.mark.parametrize('n', R.LATENT_N)
def test_latent(be, n, dim):
    for extra in (0, 7):
        R.check_latent(be, DEV, n, dim, extra)


@pytest.mark.parametrize('act', R.ACTION_ACT)
@pytest.mark.parametrize('n', R.ACTION_N)
def test_llc_action(be, n, act):
    for pitch in R.ACTION_PITCH:
        if pitch >= act:
            R.check_llc_action(be, DEV, n, act, pitch)


@pytest.mark.parametrize('T_', R.ACCUM_T)
@pytest.mark.parametrize('n', R.ACCUM_N)
def test_accum_sequences(be, n, T_):
    R.check_accum(be, DEV, n, T_, ld_l=1 if n % 2 else 128)


@pytest.mark.parametrize('term_dtype', R.KINDS)
@pytest.mark.parametrize('dones_dtype', R.KINDS)
def test_accum_flag_kinds(be, dones_dtype, term_dtype):
    R.check_accum(be, DEV, 65, 3, dones_dtype, term_dtype)


def test_accum_non_finite(be):
    gen = torch.Generator().manual_seed(3)
    R.check_accum(be, DEV, 65, 3, torch.float32, torch.uint8, case=R.special_accum_case(65, 3, gen))


@pytest.mark.parametrize('groups', ((), ('terminate',), ('logit',)))
def test_accum_nullable_groups(be, groups):
    R.check_accum(be, DEV, 65, 2, groups=groups)


# ---- what the cases promise ----------------------------------------------------------------------------------------------------
def test_fixture_conditions():
    gen = torch.Generator().manual_seed(1)
    rewards, dones, terminate, logit = R.accum_case(257, 3, gen)
    for f in (dones, terminate):
        k = f.sum(0)
        assert int((k == 0).sum()) >= 8 and int((k == 1).sum()) >= 8 and int((k == 3).sum()) >= 8
    l = logit[:, :, 0]
    assert float(l.min()) <= -30.0 and float(l.max()) >= 30.0 and float(l.min()) >= -30.0 and float(l.max()) <= 30.0
    one_minus = 1 - 1 / (1 + torch.exp(-l.double()))
    assert bool((one_minus < 1e-4).any()) and bool((one_minus > 1e-4).any())
    assert bool(((one_minus - 1e-4).abs() < 2e-8).any())                 # right at the clamp, from both sides
    mu, low, high = R.action_case(1030, 31, gen)
    fin = mu[torch.isfinite(mu)]
    assert float((fin.abs() > 1).float().mean()) >= 0.10 and bool((mu == 1).any()) and bool((mu == -1).any())
    assert bool(torch.isnan(mu).any()) and bool(torch.isinf(mu).any()) and bool((low == high).any())
    assert bool((low != -high).all())
    a, special = R.latent_actions(257, 64, gen)
    assert bool((a[special['zero']] == 0).all()) and bool((a[special['tiny']] == 1e-20).all()) and bool(torch.isnan(a[special['nan']]).any())
    assert float((a[3:].abs() > 1).float().mean()) >= 0.10


# ---- single-term wrong restatements --------------------------------------------------------------------------------------------
def _differs(a, b):
    return not torch.equal(R.bits(a), R.bits(b))


@pytest.mark.parametrize('wrong', R.WRONG)
def test_single_term_wrong_restatements_miss_a_bar(be, wrong):
    gen = torch.Generator().manual_seed(2)
    if wrong == 'normalize_before_clamp':
        a, _ = R.latent_actions(5, 64, gen)
        z = torch.empty(5, 64)
        be.hrl_latent(a, z=z)
        R.same(z[3:], R.ref_latent(a)[3:], 'the right lines')
        assert _differs(z[3:], R.ref_latent(a, wrong=wrong)[3:])
        return
    if wrong == 'clamp_after_rescale':
        mu, low, high = R.action_case(65, 31, gen)
        out = torch.empty(65, 31)
        be.hrl_llc_action(mu, low, high, out, 31)
        R.same(out, R.ref_llc_action(mu, low, high), 'the right lines')
        assert _differs(out, R.ref_llc_action(mu, low, high, wrong=wrong))
        return
    n, T_ = 65, 3
    rewards, dones, terminate, logit = R.accum_case(n, T_, gen)
    dones = dones.to(torch.float32)
    if wrong == 'reciprocal_multiply':
        # a value where x / 3 and x * RN(1 / 3) differ: the sum 5.0 (5 / 3 = 1.6666666 rounds down, 5 * 0.33333334 up)
        rewards[:, 0] = torch.tensor([1.0, 1.5, 2.5])
        x = torch.tensor(5.0)
        assert float(x / 3) != float(x * (torch.tensor(1.0) / 3))
    if wrong == 'count_ge_one':
        dones[:, 5] = torch.tensor([0.0, 0.5, 0.0])                       # an f32 flag of 0.5: count 0.5 > 0, but not >= 1
    acc, outs = torch.zeros(4, n), torch.zeros(4, n)
    for t in range(T_):
        be.hrl_accum(rewards[t], dones[t], acc, t == 0, t == T_ - 1, T_, terminate=terminate[t], rewards_out=outs[0],
                     dones_out=outs[2], terminate_out=outs[3])
    for w, differs in ((None, False), (wrong, True)):
        _, finals = R.ref_fold(list(rewards), list(dones), list(terminate), None, T_, wrong=w)
        got = (outs[0], outs[2]) if wrong != 'count_ge_one' and wrong != 'dones_last_step_only' else (outs[2],)
        want = (finals[0], finals[2]) if len(got) == 2 else (finals[2],)
        assert any(_differs(g, x) for g, x in zip(got, want)) == differs, (w, differs)


# ---- the C entries' refusals ---------------------------------------------------------------------------------------------------
def test_entry_points_refuse_without_a_launch():
    """Every refusal of the three entries.  n is checked last, so every call here carries n = 0 beside the defect under test: a
    call whose defect were missed would still be refused for its n, and nothing is ever launched."""
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ase_hip_last_error()

    def caller(fn, name, defaults):
        def call(**kw):
            a = dict(defaults)
            assert set(kw) <= set(a), kw
            a.update(kw)
            rc = getattr(lib, fn)(*a.values())
            return rc == -1 and name in err() and err()
        return call

    lat = caller('ase_hip_hrl_latent', b'hrl_latent', dict(actions=p, ld_a=64, z=p, ld_z=64, z2=p, ld_z2=64, z2_dtype=L.BF16, n=0,
                                                             dim=64, stream=None))
    for kw in ({}, dict(z=None), dict(z2=None), dict(dim=1), dict(dim=128, ld_a=128, ld_z=128, ld_z2=128), dict(z2_dtype=L.F16),
               dict(z2_dtype=L.F32), dict(z2=None, z2_dtype=77)):
        assert b'n 0' in lat(**kw), kw
    assert b'null actions' in lat(actions=None)
    assert b'neither z nor z2' in lat(z=None, z2=None)
    assert b'dim 0' in lat(dim=0) and b'dim 129' in lat(dim=129, ld_a=256, ld_z=256, ld_z2=256)
    for k in ('ld_a', 'ld_z', 'ld_z2'):
        assert b'pitch' in lat(**{k: 63}), k
    assert b'z2 dtype' in lat(z2_dtype=L.F32X3) and b'z2 dtype' in lat(z2_dtype=-1)
    assert b'n -3' in lat(n=-3)

    act = caller('ase_hip_hrl_llc_action', b'hrl_llc_action', dict(mu=p, ld_mu=64, low=p, high=p, out=p, ld_out=31, n=0, act=31,
                                                                   clip=1, stream=None))
    for kw in ({}, dict(clip=0, low=None, high=None), dict(act=1), dict(act=128, ld_mu=128, ld_out=128)):
        assert b'n 0' in act(**kw), kw
    assert b'null mu' in act(mu=None) and b'null mu' in act(out=None)
    assert b'clip without' in act(low=None) and b'clip without' in act(high=None)
    assert b'act 0' in act(act=0) and b'act 129' in act(act=129, ld_mu=256, ld_out=256)
    assert b'pitch' in act(ld_mu=30) and b'pitch' in act(ld_out=30)
    assert b'n -1' in act(n=-1)

    acc = caller('ase_hip_hrl_accum', b'hrl_accum', dict(rewards=p, dones=p, dones_kind=L.KIND_U8, terminate=p,
                                                         terminate_kind=L.KIND_I64, logit=p, ld_l=128, disc_scale=2.0, acc=p,
                                                         acc_stride=16, first=1, last=1, llc_steps=5, rewards_out=p, disc_out=p,
                                                         dones_out=p, terminate_out=p, n=0, stream=None))
    outs_none = dict(rewards_out=None, disc_out=None, dones_out=None, terminate_out=None)
    for kw in ({}, dict(terminate=None, terminate_out=None), dict(logit=None, disc_out=None), dict(last=0), dict(last=0, **outs_none),
               dict(dones_kind=L.KIND_F32, terminate_kind=L.KIND_I32), dict(llc_steps=1), dict(first=0), dict(ld_l=1),
               dict(terminate=None, terminate_out=None, terminate_kind=99)):
        assert b'n 0' in acc(**kw), kw
    for k in ('rewards', 'dones', 'acc'):
        assert b'null rewards / dones / acc' in acc(**{k: None}), k
    assert b'dones kind 4' in acc(dones_kind=4) and b'dones kind -1' in acc(dones_kind=-1)
    assert b'terminate kind 7' in acc(terminate_kind=7)
    assert b'partial terminate group' in acc(terminate=None)                                  # terminate_out without terminate
    assert b'partial terminate group' in acc(terminate_out=None)                              # last, terminate without its output
    assert b'partial terminate group' in acc(terminate=None, last=0)
    assert b'partial discriminator group' in acc(logit=None) and b'partial discriminator group' in acc(disc_out=None)
    assert b'partial discriminator group' in acc(logit=None, last=0)
    assert b'logit pitch' in acc(ld_l=0)
    assert b'llc_steps 0' in acc(llc_steps=0) and b'llc_steps -2' in acc(llc_steps=-2)
    assert b'last without' in acc(rewards_out=None) and b'last without' in acc(dones_out=None)
    assert b'acc_stride' in acc(acc_stride=15, n=16) and b'acc_stride' in acc(acc_stride=-1)
    assert b'n -5' in acc(n=-5, acc_stride=0)


def test_torch_ops_are_registered():
    import ase_amd.ops  # noqa: F401
    assert str(torch.ops.ase_hip.hrl_latent.default._schema) == 'ase_hip::hrl_latent(Tensor actions) -> Tensor'
    schema = str(torch.ops.ase_hip.hrl_accum.default._schema)
    for name in ('rewards_out', 'disc_out', 'dones_out', 'terminate_out'):
        assert f'!)? {name}' in schema, (name, schema)
    assert '!) acc' in schema and schema.endswith('-> ()')
    assert 'hrl_llc_action(Tensor mu, Tensor low, Tensor high, SymInt act, bool clip) -> Tensor' in \
        str(torch.ops.ase_hip.hrl_llc_action.default._schema)
    for name in ('hrl_latent(', 'hrl_llc_action(', 'hrl_accum('):
        assert name in ase_amd.ops.__doc__
    with pytest.raises(NotImplementedError):                               # no CPU kernel: the product has no fallback
        torch.ops.ase_hip.hrl_latent(torch.zeros(4, 8))


def test_host_addresses_never_reach_the_launch():
    """HipBackend's three methods take raw addresses: a tensor that is not on the backend's GPU is refused by an assertion before
    the library is called (here: a backend object without a GPU behind it, so nothing can run)."""
    from ase_amd.backend import HipBackend
    hb = HipBackend.__new__(HipBackend)
    hb.device = torch.device('cuda:0')
    hb.lib = None
    x = torch.zeros(4, 8)
    with pytest.raises(AssertionError, match='actions'):
        hb.hrl_latent(x, z=x.clone())
    with pytest.raises(AssertionError, match='mu'):
        hb.hrl_llc_action(x, torch.zeros(8), torch.zeros(8), x.clone(), 8)
    with pytest.raises(AssertionError, match='rewards'):
        hb.hrl_accum(torch.zeros(4), torch.zeros(4), torch.zeros(4, 4), True, False, 3)


# ---- the agents on the stand-in ------------------------------------------------------------------------------------------------
def _golden_agent(golden_dir, key, llc_steps=None, cls=agents.HRLAgent, **extra):
    """tests/test_boundary_emu.py::test_hrl_env_step_matches_reference_golden's construction."""
    G = torch.load(os.path.join(golden_dir, 'hrl_step.pt'), weights_only=False)
    sp, Lc, Hc = G['spec'], G['llc'], G['hlc']
    spec = EnvSpec(num_envs=sp['num_envs'], horizon=Hc['cfg']['horizon_length'], obs_size=sp['obs_size'], act_size=sp['act_size'],
                   amp_obs_size=sp['amp_obs_size'], latent_dim=Lc['cfg']['latent_dim'], episode_length=G['episode_length'])
    env = SyntheticVecEnv(spec, seed=G['env_seed'], task_obs_size=sp['task'], device=DEV)
    llc_ckpt = {'model': Lc['sd'], 'running_mean_std': Lc['running_mean_std'], 'amp_input_mean_std': Lc['amp_input_mean_std'],
                'reward_mean_std': Lc['reward_mean_std'], 'epoch': 0, 'frame': 0,
                'optimizer': {'state': {}, 'param_groups': [{'lr': Lc['cfg']['learning_rate']}]}}
    b = BUILDERS['ppo']()
    b.load(Hc['net'])
    cfg = dict(Hc['cfg'])
    cfg.update(network=T.models.ModelHRLContinuous(b), num_actors=spec.num_envs, device=DEV, backend=EmuHrlStep(), precision='f32',
               vec_env=env, print_stats=False, env_info={'observation_space': env.observation_space, 'action_space': env.action_space},
               llc_config={'params': {'network': Lc['net'], 'config': dict(Lc['cfg'])}}, llc_checkpoint=llc_ckpt,
               llc_steps=G['llc_steps'] if llc_steps is None else llc_steps, device_llc_step=key)
    cfg.update(extra)
    if cls is players.HRLPlayer:
        cfg.update(env_info=None, player={'games_num': 1, 'print_stats': False})
    return cls('hrl', cfg) if cls is agents.HRLAgent else cls(cfg), env, G


def _record_actions(env):
    seen, step = [], env.step

    def recording(actions):
        seen.append(actions.clone())
        return step(actions)
    env.step = recording
    return seen


def test_agent_with_the_key_matches_the_reference_golden(golden_dir, monkeypatch):
    ag, env, G = _golden_agent(golden_dir, True)
    ag.obs = ag.env_reset()
    assert torch.equal(ag.obs['obs'], G['obs0'])
    R.InnerLoopGuard(monkeypatch, ag, env, [ag.backend, ag._llc_agent.backend])
    obs1, rewards, dones, infos = ag.env_step(G['actions'])
    monkeypatch.undo()
    assert ag.backend.hrl_calls == {'latent': 1, 'llc_action': G['llc_steps'], 'accum': G['llc_steps']}
    assert torch.allclose(env.last_actions, G['env_last_actions'], rtol=1e-4, atol=2e-5)
    assert torch.equal(obs1['obs'], G['obs1'])
    assert torch.allclose(rewards, G['rewards']) and rewards.shape == G['rewards'].shape
    assert torch.equal(dones, G['dones'].float()) and torch.equal(infos['terminate'], G['terminate'].float())
    assert torch.allclose(infos['disc_rewards'], G['disc_rewards'], rtol=1e-4, atol=2e-5)
    assert infos['disc_rewards'].shape == G['disc_rewards'].shape


@pytest.mark.parametrize('llc_steps', (2, 3, 4, 5))
def test_agent_with_the_key_equals_the_default_path(golden_dir, monkeypatch, llc_steps):
    """Two high-level steps on twin environments: obs, dones, terminate and the actions that reach the environment bitwise,
    rewards / disc_rewards at the bar of tests/ref_hrl_step.py; the default path never touches the entries."""
    ag, env, G = _golden_agent(golden_dir, True, llc_steps)
    tw, tenv, _ = _golden_agent(golden_dir, False, llc_steps)
    acts, tacts = _record_actions(env), _record_actions(tenv)
    R.InnerLoopGuard(monkeypatch, ag, env, [ag.backend, ag._llc_agent.backend])
    gen = torch.Generator().manual_seed(4)
    for a in (ag, tw):
        a.obs = a.env_reset()
    for step in range(2):
        actions = torch.randn(G['actions'].shape, generator=gen) * 1.5
        o1, r1, d1, i1 = ag.env_step(actions)
        o2, r2, d2, i2 = tw.env_step(actions)
        ag.obs, tw.obs = o1, o2
        for name, x, y in (('obs', o1['obs'], o2['obs']), ('dones', d1, d2), ('terminate', i1['terminate'], i2['terminate'])):
            R.same(x, y, f'{name} step {step}')
        assert r1.shape == r2.shape and i1['disc_rewards'].shape == i2['disc_rewards'].shape and d1.shape == d2.shape
        R.agent_reward_bar(r1, r2, llc_steps, f'rewards step {step}')
        R.agent_reward_bar(i1['disc_rewards'], i2['disc_rewards'], llc_steps, f'disc_rewards step {step}')
    monkeypatch.undo()
    assert len(acts) == len(tacts) == 2 * llc_steps
    for k, (x, y) in enumerate(zip(acts, tacts)):
        R.same(x, y, f'environment action {k}')
    assert ag.backend.hrl_calls == {'latent': 2, 'llc_action': 2 * llc_steps, 'accum': 2 * llc_steps}
    assert tw.backend.hrl_calls == {'latent': 0, 'llc_action': 0, 'accum': 0}


@pytest.mark.parametrize('llc_steps', (3, 4))
def test_player_with_the_key_equals_the_default_path(golden_dir, monkeypatch, llc_steps):
    pl, env, G = _golden_agent(golden_dir, True, llc_steps, cls=players.HRLPlayer)
    tw, tenv, _ = _golden_agent(golden_dir, False, llc_steps, cls=players.HRLPlayer)
    acts, tacts = _record_actions(env), _record_actions(tenv)
    R.InnerLoopGuard(monkeypatch, pl, env, [pl.backend, pl._llc_agent.backend])
    o1, o2 = pl.env_reset(), tw.env_reset()
    action = torch.clamp(G['actions'] * 1.5, -1.0, 1.0)                  # what HRLPlayer.get_action hands over
    for step in range(2):
        o1, r1, d1, i1 = pl.env_step(env, o1, action)
        o2, r2, d2, i2 = tw.env_step(tenv, o2, action)
        R.same(o1['obs'], o2['obs'], 'obs')
        R.same(d1, d2, 'dones')
        assert r1.shape == r2.shape and i1['disc_rewards'].shape == i2['disc_rewards'].shape
        R.agent_reward_bar(r1, r2, llc_steps, 'player rewards')
        R.agent_reward_bar(i1['disc_rewards'], i2['disc_rewards'], llc_steps, 'player disc_rewards')
    monkeypatch.undo()
    for k, (x, y) in enumerate(zip(acts, tacts)):
        R.same(x, y, f'environment action {k}')
    assert pl.backend.hrl_calls['accum'] == 2 * llc_steps and tw.backend.hrl_calls['accum'] == 0


def test_key_composes_with_device_rollout(golden_dir, tmp_path, monkeypatch):
    """play_steps with both keys against device_rollout alone: the finals are the agent's buffers, rollout_store takes the f32
    flags, and every experience field agrees."""
    cfg, env, llc, GL, GH = T._hrl_setup(golden_dir, tmp_path)
    exps = []
    for key in (True, False):
        e = SyntheticVecEnv(env.spec, seed=11, task_obs_size=5, device=DEV)
        torch.manual_seed(0)                         # the high-level net's initial weights
        ag = agents.HRLAgent('hrl', dict(cfg, vec_env=e, backend=EmuHrlStep(), device_rollout=True, device_llc_step=key))
        if key:
            R.InnerLoopGuard(monkeypatch, ag, e, [ag.backend, ag._llc_agent.backend])
        ag.play_steps()
        monkeypatch.undo()
        exps.append(ag.experience)
    for k in exps[0]:
        if k in ('rewards', 'disc_rewards'):
            R.agent_reward_bar(exps[0][k], exps[1][k], 3, k)
        else:
            R.same(exps[0][k], exps[1][k], k)


def test_frozen_statistics_are_dropped_when_the_statistics_change(golden_dir):
    ag, env, G = _golden_agent(golden_dir, True)
    llc = ag._llc_agent
    e = llc.engine
    assert set(e._frozen) == {'obs', 'amp'}
    mean0 = e.frozen_stats('obs')[0].clone()
    w = llc.get_stats_weights()
    w['running_mean_std']['running_mean'] = w['running_mean_std']['running_mean'] + 1.0
    llc.set_stats_weights(w)
    assert e._frozen == {}
    assert torch.allclose(e.frozen_stats('obs')[0], mean0 + 1.0)
    llc.set_train()
    assert e._frozen == {}
    e.frozen_stats('amp')
    llc.set_full_state_weights(llc.get_full_state_weights())
    assert e._frozen == {}


def test_key_refusals(golden_dir, monkeypatch):
    ag, env, G = _golden_agent(golden_dir, True)
    monkeypatch.setattr(ag._llc_agent.engine, 'mu_tanh', True)
    with pytest.raises(AssertionError, match='mu_tanh'):
        ag._check_device_llc_step()
    monkeypatch.undo()
    monkeypatch.setattr(ag, '_latent_dim', 129)
    with pytest.raises(AssertionError, match='latent_dim 129'):
        ag._check_device_llc_step()
    monkeypatch.undo()
    monkeypatch.setattr(ag._llc_agent, 'actions_low', torch.zeros(129))
    with pytest.raises(AssertionError, match='action width 129'):
        ag._check_device_llc_step()
    monkeypatch.undo()
    monkeypatch.setattr(SyntheticVecEnv, 'returns_numpy', True, raising=False)
    with pytest.raises(AssertionError, match='numpy'):
        _golden_agent(golden_dir, True)
    with pytest.raises(AssertionError, match='numpy'):
        _golden_agent(golden_dir, True, cls=players.HRLPlayer)
    monkeypatch.undo()
    # an environment that hands numpy over without declaring it is refused at the step
    step = env.step

    def numpy_step(actions):
        o, r, d, i = step(actions)
        return o.numpy(), r, d, i
    env.step = numpy_step
    ag.obs = ag.env_reset()
    with pytest.raises(AssertionError, match='tensors only'):
        ag.env_step(G['actions'])
    from tests.emu_rollout_store import EmuRolloutStore
    with pytest.raises(AssertionError, match='backend with hrl_latent'):
        _golden_agent(golden_dir, True, backend=EmuRolloutStore())
