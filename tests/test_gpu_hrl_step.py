"""The HRL inner loop's glue on the MI355X: ``ase_hip_hrl_latent`` / ``ase_hip_hrl_llc_action`` /
``ase_hip_hrl_accum`` through ``HipBackend``, ``torch.ops.ase_hip``, a launch program and the agents' ``device_llc_step``.

The bars (tests/ref_hrl_step.py): z bitwise the device's own normalize_rows(clamp), z2 bitwise gather_rows' conversion, the
environment's action bitwise the CPU f32 run of rescale_actions(clamp), the four accumulator rows after every call and the four
outputs after the last bitwise the f32 run of the reference's lines on the device's own per-step discriminator rewards - all
inside NaN-filled allocations of a wider pitch whose every guard word is looked at after each launch; z and disc_out against
f64 at the bars written down there.  ASE_HRL_STEP_REPORT=<file> writes the counts and the observed maxima (COVERAGE.md N13)."""
import json
import os

import pytest
import torch

from tests import ref_hrl_step as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    yield HipBackend('cuda:0')
    out = os.environ.get('ASE_HRL_STEP_REPORT')
    if out:
        with open(out, 'w') as f:
            json.dump(R.report(), f, indent=1)


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


def test_torch_ops_equal_the_backend_calls(be):
    import ase_amd.ops  # noqa: F401
    gen = torch.Generator().manual_seed(21)
    a, _ = R.latent_actions(65, 64, gen)
    a = a.to(DEV)
    z = torch.empty(65, 64, device=DEV)
    be.hrl_latent(a, z=z)
    R.same(torch.ops.ase_hip.hrl_latent(a), z, 'hrl_latent op')
    mu, low, high = (t.to(DEV) for t in R.action_case(65, 31, gen))
    head = torch.zeros(65, 64, device=DEV)
    head[:, :31] = mu
    for clip in (True, False):
        out = torch.empty(65, 31, device=DEV)
        be.hrl_llc_action(head, low, high, out, 31, clip=clip)
        R.same(torch.ops.ase_hip.hrl_llc_action(head, low, high, 31, clip), out, f'hrl_llc_action op clip {clip}')
    rewards, dones, terminate, logit = R.accum_case(65, 2, gen, ld_l=4)
    res = []
    for op in (True, False):
        acc, outs = torch.full((4, 65), R.NAN, device=DEV), torch.full((4, 65), R.NAN, device=DEV)
        for t in range(2):
            args = (rewards[t].to(DEV), dones[t].to(torch.uint8).to(DEV), terminate[t].to(torch.bool).to(DEV), logit[t].to(DEV))
            if op:
                torch.ops.ase_hip.hrl_accum(args[0], args[1], args[2], args[3], R.DISC_SCALE, acc, t == 0, t == 1, 2, outs[0],
                                            outs[1], outs[2], outs[3])
            else:
                be.hrl_accum(args[0], args[1], acc, t == 0, t == 1, 2, terminate=args[2], logit=args[3], disc_scale=R.DISC_SCALE,
                             rewards_out=outs[0], disc_out=outs[1], dones_out=outs[2], terminate_out=outs[3])
        res.append((acc, outs))
    R.same(res[0][0], res[1][0], 'hrl_accum op: accumulator')
    R.same(res[0][1], res[1][1], 'hrl_accum op: outputs')
    assert not bool(torch.isnan(res[0][1]).any())


# ---- the agents ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def boundary(monkeypatch):
    import tests.test_boundary_emu as T
    from ase_amd.backend import HipBackend
    monkeypatch.setattr(T, '_DEV', 'cuda:0')
    monkeypatch.setattr(T, '_BE', lambda: HipBackend('cuda:0'))
    return T


def test_launch_program_holds_an_inner_step(be, boundary, golden_dir):
    """One inner step's entries recorded once - recording executes nothing - and replayed with the inputs rewritten: bitwise the
    eager twin; the program holds one entry per dense layer plus two before the environment's step (normalise, hrl_llc_action)
    and two after it (normalise, hrl_accum)."""
    T = boundary
    G = T._load(golden_dir, 'ase')
    ag, _ = T._agent(G, T._env(G))
    e, n, task = ag.engine, G['spec']['num_envs'], 5
    gen = torch.Generator().manual_seed(33)
    full = torch.zeros(n, e.obs + task, device=DEV)                     # the HRL observation: the LLC's part is a strided view
    amp = torch.zeros(n, e.amp, device=DEV)
    actions = torch.zeros(n, e.z, device=DEV)
    low, high = ag.actions_low, ag.actions_high
    rewards, dones = torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    terminate = torch.zeros(n, dtype=torch.bool, device=DEV)

    def fill():
        full.copy_(torch.randn(full.shape, generator=gen))
        amp.copy_(torch.randn(amp.shape, generator=gen))
        actions.copy_(torch.randn(actions.shape, generator=gen) * 1.5)
        rewards.copy_(torch.randn(n, generator=gen))
        dones.copy_((torch.rand(n, generator=gen) < 0.4).to(torch.uint8))
        terminate.copy_(torch.rand(n, generator=gen) < 0.3)

    def before(out):
        MU = e.policy_mu_frozen(full[:, :e.obs])
        be.hrl_llc_action(MU, low, high, out, e.act, clip=True)

    def after(acc, outs):
        HD, _ = e.amp_heads(amp, frozen=True, want_enc=False)
        be.hrl_accum(rewards, dones, acc, True, True, 1, terminate=terminate, logit=HD, disc_scale=R.DISC_SCALE,
                     rewards_out=outs[0], disc_out=outs[1], dones_out=outs[2], terminate_out=outs[3])
    bufs = [(torch.full((n, e.act), R.NAN, device=DEV), torch.full((4, n), R.NAN, device=DEV), torch.full((4, n), R.NAN, device=DEV))
            for _ in range(2)]
    fill()
    be.hrl_latent(actions, z2=e.style_input(n))
    before(bufs[1][0])                                                  # eager once: scratch and the frozen statistics exist
    after(bufs[1][1], bufs[1][2])
    torch.cuda.synchronize()
    progs = [be.prog_create(), be.prog_create()]
    be.prog_begin(progs[0])
    try:
        before(bufs[0][0])
    finally:
        be.prog_end(progs[0])
    be.prog_begin(progs[1])
    try:
        after(bufs[0][1], bufs[0][2])
    finally:
        be.prog_end(progs[1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(bufs[0][0]).all()) and bool(torch.isnan(bufs[0][2]).all())          # recording executed nothing
    assert be.prog_size(progs[0]) == len(e.style) + len(e.actor) + 1 + 2
    assert be.prog_size(progs[1]) == len(e.disc) + 1 + 2
    for rep in range(2):
        fill()
        be.hrl_latent(actions, z2=e.style_input(n))
        be.prog_launch(progs[0])
        be.prog_launch(progs[1])
        before(bufs[1][0])
        after(bufs[1][1], bufs[1][2])
        torch.cuda.synchronize()
        for a, b, what in zip(bufs[0], bufs[1], ('action', 'accumulator', 'outputs')):
            R.same(a, b, f'replay {rep} against the eager twin: {what}')
        assert not bool(torch.isnan(bufs[0][0]).any()) and not bool(torch.isnan(bufs[0][2]).any())
    for p in progs:
        be.prog_destroy(p)


@pytest.fixture(scope='module')
def hrl64(golden_dir, tmp_path_factory):
    """_hrl_setup on the GPU with 64 environments for the high-level agent, once for the module (it trains the LLC an epoch)."""
    import tests.test_boundary_emu as T
    from ase_amd.backend import HipBackend
    keep = (T._DEV, T._BE, T._load)

    def load64(golden_dir, kind):
        G = keep[2](golden_dir, kind)
        return dict(G, spec=dict(G['spec'], num_envs=64)) if kind == 'ppo' else G
    T._DEV, T._BE, T._load = 'cuda:0', (lambda: HipBackend('cuda:0')), load64
    try:
        cfg, env, llc, GL, GH = T._hrl_setup(golden_dir, tmp_path_factory.mktemp('hrl64'))
    finally:
        T._DEV, T._BE, T._load = keep
    assert env.num_envs == 64 and cfg['llc_steps'] == 3
    return cfg, env.spec, GL


@pytest.mark.parametrize('device_rollout', (False, True))
def test_agent_trains_an_epoch_with_the_key(boundary, hrl64, monkeypatch, device_rollout):
    """64 environments, the tiny nets, llc_steps 3: one train_epoch with the key, normalize_rows / gather_rows / rms_finalize /
    torch.clamp raising inside the inner loop, against a twin on the default path - experience bitwise but for rewards /
    disc_rewards (the x / 3 bar), the LLC's weights unchanged."""
    from ase_amd.learning import agents
    from ase_amd.synthetic import SyntheticVecEnv
    T = boundary
    cfg, spec, GL = hrl64
    exps = []
    for key in (True, False):
        e = SyntheticVecEnv(spec, seed=11, task_obs_size=5, device='cuda:0')
        torch.manual_seed(0)                                            # the high-level net's initial weights
        ag = agents.HRLAgent('hrl', dict(cfg, vec_env=e, backend=T._BE(), device_rollout=device_rollout, device_llc_step=key))
        w_llc = ag._llc_agent.model.a2c_network.flat_params.clone()
        ag._init_train()
        if key:
            with monkeypatch.context() as m:
                R.InnerLoopGuard(m, ag, e, [ag.backend, ag._llc_agent.backend])
                info = ag.train_epoch()
        else:
            info = ag.train_epoch()
        torch.cuda.synchronize()
        assert e.steps == ag.horizon_length * 3
        assert torch.equal(w_llc, ag._llc_agent.model.a2c_network.flat_params)
        assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in info['actor_loss'])
        exps.append({k: v.clone() for k, v in ag.experience.items()})
    assert set(exps[0]) == set(exps[1])
    for k in exps[0]:
        if k in ('rewards', 'disc_rewards'):
            R.agent_reward_bar(exps[0][k], exps[1][k], 3, k)
        else:
            R.same(exps[0][k], exps[1][k], k)
    assert int(exps[0]['dones'].sum()) > 0


def test_player_with_the_key(boundary, hrl64, monkeypatch):
    from ase_amd.learning import players
    from ase_amd.synthetic import SyntheticVecEnv
    T = boundary
    cfg, spec, GL = hrl64
    res = []
    gen = torch.Generator().manual_seed(8)
    action = torch.clamp(torch.randn(64, GL['cfg']['latent_dim'], generator=gen) * 1.5, -1.0, 1.0).to('cuda:0')
    for key in (True, False):
        e = SyntheticVecEnv(spec, seed=4, task_obs_size=5, device='cuda:0')
        torch.manual_seed(0)
        pl = players.HRLPlayer(dict(cfg, vec_env=e, env_info=None, backend=T._BE(), device_llc_step=key,
                                    player={'games_num': 1, 'print_stats': False}))
        seen, step = [], e.step

        def recording(actions, seen=seen, step=step):
            seen.append(actions.clone())
            return step(actions)
        e.step = recording
        obs = pl.env_reset()
        with monkeypatch.context() as m:
            if key:
                R.InnerLoopGuard(m, pl, e, [pl.backend, pl._llc_agent.backend])
            o, r, d, i = pl.env_step(e, obs, action)
        torch.cuda.synchronize()
        res.append((o['obs'].clone(), d.clone(), torch.stack(seen), r.clone(), i['disc_rewards'].clone()))
    for k, what in enumerate(('obs', 'dones', 'environment actions')):
        R.same(res[0][k], res[1][k], what)
    assert res[0][3].shape == res[1][3].shape and res[0][4].shape == res[1][4].shape
    R.agent_reward_bar(res[0][3], res[1][3], 3, 'player rewards')
    R.agent_reward_bar(res[0][4], res[1][4], 3, 'player disc_rewards')
