"""Learned action log-std (rl_games learn_sigma: the state-independent vector of fixed_sigma True, the per-state sigma head of
fixed_sigma False) on CPU through the op emulator, against goldens the unmodified reference recorded with entropy_coef 0.01
(scripts/make_golden_sigma.py): builder layout, two-epoch replays, sharded data parallelism, and the frozen layout unchanged."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ase_amd import lib as L
from tests.emu_learned_sigma import LearnedSigmaEmu
from tests.helpers import build_net, close_entry
from tests.test_agent_emu import make_agent, replay_epochs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIGMA_GOLDENS = ['ase_lsig_tiny', 'ase_sighead_tiny', 'amp_sighead_tiny', 'ppo_sighead_tiny']


def _load(name):
    return torch.load(os.path.join(GOLDEN, name + '.pt'), weights_only=False)


@pytest.mark.parametrize('name', SIGMA_GOLDENS)
def test_builder_matches_the_reference_layout(name):
    G = _load(name)
    fixed = G['net']['space']['continuous']['fixed_sigma']
    net = build_net(G)
    assert net.sigma_mode == ('vector' if fixed else 'head')
    sd = net.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in G['init_shapes'].items()}
    assert [k for k, p in net.named_parameters() if p.requires_grad] == G['trainable']
    A = G['spec']['act_size']
    if fixed:
        assert net.sigma.requires_grad and tuple(net.sigma.shape) == (A,)
    else:
        assert net.sigma.weight.requires_grad and net.sigma.bias.requires_grad
    # the builder's own initialisers (not the golden's state): the reference's sigma_init after every Linear's, biases zero
    from tests.helpers import BUILDERS
    b = BUILDERS[G['kind']]()
    b.load(G['net'])
    kw = dict(actions_num=A, input_shape=(G['spec']['obs_size'],), num_seqs=1, value_size=1)
    if G['kind'] in ('amp', 'ase'):
        kw['amp_input_shape'] = (G['spec']['amp_obs_size'],)
    if G['kind'] == 'ase':
        kw['ase_latent_shape'] = (G['cfg']['latent_dim'],)
    fresh = b.build(G['kind'], **kw)
    bounds = G['init_bounds']
    if fixed:
        assert torch.all(fresh.sigma == bounds['sigma']['const'])
    else:
        w = fresh.sigma.weight
        assert float(w.abs().max()) <= 0.02 and float(w.std()) > 0.0 and torch.all(fresh.sigma.bias == 0)
    # trainable tensors first in the flat buffer, in the reference's parameter order (the checkpoint / Adam order)
    ps = fresh.param_slices
    assert sorted(G['trainable'], key=lambda k: ps[k][0]) == G['trainable']
    assert fresh.trainable_numel == sum(p.numel() for p in fresh.parameters() if p.requires_grad)
    assert all(ps[k][0] < fresh.trainable_numel for k in G['trainable'])


def test_sigma_activation_other_than_none_is_refused():
    G = _load('ase_sighead_tiny')
    import copy
    G = dict(G)
    G['net'] = copy.deepcopy(G['net'])
    G['net']['space']['continuous']['sigma_activation'] = 'tanh'
    with pytest.raises(AssertionError, match='sigma_activation'):
        build_net(G)


@pytest.mark.parametrize('name', SIGMA_GOLDENS)
def test_replay_learned_sigma_emulated(name):
    G = _load(name)
    ag = make_agent(G, LearnedSigmaEmu())
    replay_epochs(G, ag, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25)


@pytest.mark.parametrize('name', ['ase_lsig_tiny', 'ase_sighead_tiny'])
def test_first_step_sigma_gradient_emulated(name):
    G = _load(name)
    ag = make_agent(G, LearnedSigmaEmu())
    captured = {}
    orig = ag.engine.phase_finish

    def grab(*a, **kw):
        r = orig(*a, **kw)
        if not captured:
            captured.update(ag.engine.export_grads())
        return r
    ag.engine.phase_finish = grab
    replay_epochs(G, ag, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25, check=False, max_steps=1)
    fg = G['epochs'][0]['first_grads']
    seed = G.get('sample', {}).get('seed', 0)
    keys = ['sigma'] if name == 'ase_lsig_tiny' else ['sigma.weight', 'sigma.bias']
    for k in keys:
        close_entry(k, captured[k], fg[k], 1e-4, 1e-6, seed, 'first-step gradient ' + k)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, name, out):
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    G = _load(name)
    ag = make_agent(G, LearnedSigmaEmu(), world_size=world, rank=rank)
    replay_epochs(G, ag, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25, check=True)
    if rank == 0:
        torch.save({'flat': ag.model.a2c_network.flat_params.clone()}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize('name', ['ase_lsig_tiny', 'ase_sighead_tiny'])
def test_two_ranks_shard_equal_one_rank(name, tmp_path):
    G = _load(name)
    ag1 = make_agent(G, LearnedSigmaEmu())
    replay_epochs(G, ag1, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25)
    out = str(tmp_path / 'r0.pt')
    mp.spawn(_worker, args=(2, _free_port(), name, out), nprocs=2, join=True)
    r = torch.load(out)
    assert torch.allclose(r['flat'], ag1.model.a2c_network.flat_params, rtol=1e-5, atol=G['cfg']['learning_rate'] * 0.25)


@pytest.mark.parametrize('name', ['ase_tiny', 'ppo_tiny'])
def test_frozen_layout_unchanged(name):
    """A frozen log-std keeps the flat layout, the trainable count and the Adam table: sigma after every trainable scalar,
    one (weight, bias) row per Linear, the mu head alone in its group."""
    G = _load(name)
    ag = make_agent(G, LearnedSigmaEmu())
    net, eng = ag.model.a2c_network, ag.engine
    assert net.sigma_mode == 'frozen' and eng.ls_mode == L.LS_FROZEN
    assert not net.sigma.requires_grad
    assert eng.n_train == sum(p.numel() for p in net.parameters() if p.requires_grad)
    o, shp = net.param_slices['sigma']
    assert o == eng.n_train and o + shp[0] == net.flat_params.numel()
    assert eng.mu_head.parts == [('mu', G['spec']['act_size'], 0)] and eng.mu_head.n_pad == 64
    eng._build_apply_desc()
    n_lin = sum(1 for m in net.modules() if isinstance(m, torch.nn.Linear))
    assert len(eng._apply_items) == n_lin and all(it[0].numel() > 0 for it in eng._apply_items)
    assert eng.glogstd is None


def test_vector_row_sits_in_the_policy_bucket():
    G = _load('ase_lsig_tiny')
    ag = make_agent(G, LearnedSigmaEmu())
    eng, net = ag.engine, ag.model.a2c_network
    eng._build_apply_desc()
    a, b, lo, hi = eng._apply_groups['policy']
    o, _ = net.param_slices['sigma']
    rows = [i for i, it in enumerate(eng._apply_items) if it[0].numel() == 0]
    assert rows == [b - 1] and lo <= o < hi and o + G['spec']['act_size'] <= hi
    assert int(eng._apply_desc[b - 1, 2]) == 0 and int(eng._apply_desc[b - 1, 11]) == 0     # k_real 0, no weight tiles
