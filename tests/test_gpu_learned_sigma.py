"""Learned action log-std on the MI355X: ase_hip_ppo_head's LS_VECTOR / LS_ROWS modes against f64 autograd of the reference's
loss expressions (and bit-identity of the frozen mode), the per-row log-std of ase_hip_sample_actions, and the agents' updates
against the goldens the unmodified reference recorded with learn_sigma (scripts/make_golden_sigma.py)."""
import math
import os

import pytest
import torch

from ase_amd import lib as L
from tests.helpers import close, close_entry
from tests.ref_heads import _head_inputs, _reference
from tests.test_agent_emu import check_rollout_inference, make_agent, regenerate, replay_epochs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIGMA_GOLDENS = ['ase_lsig_tiny', 'ase_sighead_tiny', 'amp_sighead_tiny', 'ppo_sighead_tiny']


def _load(name):
    return torch.load(os.path.join(GOLDEN, name + '.pt'), weights_only=False)


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend()


# ------------------------------------------------------------------------------------------------ the loss head
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize('A', [31, 64])
@pytest.mark.parametrize('rows', [False, True])
@pytest.mark.parametrize('variant', ['plain', 'masked_div', 'tanh_clip'])
@pytest.mark.parametrize('ec', [0.0, 0.01])
def test_ppo_head_learned_logstd_against_autograd(be, dtype, A, rows, variant, ec):
    M, Z = 300, 16
    masked = variant == 'masked_div'
    div_on = variant == 'masked_div'
    mu_tanh = clip_value = variant == 'tanh_clip'
    e_clip, cc, bc, dc, dt = 0.2, 5.0, 10.0, 0.01, 1.0
    mu, ls_rows, ls_vec, mb, new_z, value = _head_inputs(M, A, Z, 1234 + A, div_on)
    ls = ls_rows if rows else ls_vec
    stats_r, gmu_r, gls_r, gv_r = _reference(mu, ls, mb, new_z, value, M, A, masked, div_on, mu_tanh, clip_value, e_clip, cc, bc,
                                              dc, dt, ec)
    dev = 'cuda'
    R = mu.shape[0]
    # the engine's layout: [mu | log-std] stacked in one padded head output, the log-std at column 64
    MU = torch.zeros(R, 128, device=dev)
    MU[:, :A] = mu.to(dev)
    if rows:
        MU[:M, 64:64 + A] = ls_rows.to(dev)
    ls_dev = MU[:, 64:64 + A] if rows else ls_vec.to(dev)
    mbd = {k: v.to(dev).contiguous() for k, v in mb.items()}
    if not masked:
        mbd.pop('rand_action_mask')
    acc = torch.zeros(L.ACC_COUNT, dtype=torch.float64, device=dev)
    if masked:
        be.reduce_sum(mbd['rand_action_mask'], M, False, acc, L.ACC_MASK_SUM)
    dMU = torch.full((R, 128), 7.0, dtype=dtype, device=dev)            # every column the kernel owns gets written
    dV = torch.zeros(M, 64, dtype=dtype, device=dev)
    V = torch.zeros(M, 64, device=dev)
    V[:, 0] = value.view(-1).to(dev)
    db_mu, db_v, db_ls = torch.zeros(A, device=dev), torch.zeros(1, device=dev), torch.zeros(A, device=dev)
    gs = 64.0 if dtype == torch.float16 else 1.0
    be.ppo_head(MU, V, mbd, new_z.to(dev) if div_on else None, ls_dev, dMU, dV, db_mu, db_v, acc, M, M, A, Z if div_on else 0,
                masked, div_on, mu_tanh, clip_value, e_clip, cc, bc, dc, dt, grad_scale=gs,
                ls_mode=L.LS_ROWS if rows else L.LS_VECTOR, d_logstd=dMU[:, 64:], db_logstd=db_ls, entropy_coef=ec)
    torch.cuda.synchronize()
    den = float(acc[L.ACC_MASK_SUM]) if masked else float(M)
    stats = torch.tensor([float(acc[L.ACC_A_LOSS]) / den, float(acc[L.ACC_C_LOSS]) / M, float(acc[L.ACC_B_LOSS]) / den,
                          float(acc[L.ACC_ENTROPY]) / den, float(acc[L.ACC_CLIPPED]) / den, float(acc[L.ACC_KL]) / M])
    tol = {torch.float32: 2e-4, torch.float16: 3e-3, torch.bfloat16: 2e-2}[dtype]
    close(stats, stats_r, 1e-4, 1e-6, 'stats')
    got_mu = dMU[:, :A].float().cpu() / gs
    scale = float(gmu_r.abs().max())
    close(got_mu, gmu_r.float(), tol, tol * scale, 'd_mu')
    gls_rows = dMU[:M, 64:64 + A].float().cpu() / gs
    ref_rows = gls_r if rows else None
    if rows:
        close(gls_rows, ref_rows.float(), tol, tol * float(ref_rows.abs().max()), 'd_logstd rows')
        close(db_ls.cpu(), ref_rows.sum(0).float(), tol, tol * float(ref_rows.abs().max()) * 4, 'd_logstd column sums')
    else:
        close(gls_rows.sum(0), gls_r.float(), tol * 4, tol * float(gls_r.abs().max()), 'd_logstd rows (sum)')
        close(db_ls.cpu(), gls_r.float(), tol, tol * float(gls_r.abs().max()), 'vector gradient')
    if div_on:
        assert torch.all(dMU[M:, 64:64 + A].float() == 0), 'the diversity rows carry no log-std gradient'
    assert torch.all(dMU[:, A:64].float() == 7.0) and torch.all(dMU[:, 64 + A:].float() == 7.0), 'padding columns untouched'
    close(db_mu.cpu(), gmu_r.sum(0).float(), tol, tol * scale * 4, 'db_mu')
    close(dV[:, 0].float().cpu() / gs, gv_r.view(-1).float(), tol, tol * float(gv_r.abs().max()), 'd_value')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize('A', [31, 64])
def test_ppo_head_frozen_mode_is_bit_identical(be, dtype, A):
    """The defaults of the new keyword arguments are today's call: every output bit-identical to an explicit LS_FROZEN call with
    unused learned operands.  (M = 200 rows: one folding workgroup, so the f64 sums have one order and compare bitwise too.)"""
    M, Z = 200, 16
    mu, ls_rows, ls_vec, mb, new_z, value = _head_inputs(M, A, Z, 99 + A, True)
    dev = 'cuda'
    mbd = {k: v.to(dev).contiguous() for k, v in mb.items()}
    MU = torch.zeros(2 * M, 64, device=dev)
    MU[:, :A] = mu.to(dev)
    V = torch.zeros(M, 64, device=dev)
    V[:, 0] = value.view(-1).to(dev)
    outs = []
    for kw in ({}, dict(ls_mode=L.LS_FROZEN, entropy_coef=0.5)):
        acc = torch.zeros(L.ACC_COUNT, dtype=torch.float64, device=dev)
        be.reduce_sum(mbd['rand_action_mask'], M, False, acc, L.ACC_MASK_SUM)
        dMU, dV = torch.zeros(2 * M, 64, dtype=dtype, device=dev), torch.zeros(M, 64, dtype=dtype, device=dev)
        db_mu, db_v = torch.zeros(A, device=dev), torch.zeros(1, device=dev)
        be.ppo_head(MU, V, mbd, new_z.to(dev), ls_vec.to(dev), dMU, dV, db_mu, db_v, acc, M, M, A, Z, True, True, False, False,
                    0.2, 5.0, 10.0, 0.01, 1.0, grad_scale=1.0, **kw)
        outs.append((acc.clone(), dMU.clone(), dV.clone(), db_mu.clone(), db_v.clone()))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a.view(-1).view(torch.uint8) if a.dtype != torch.float64 else a, b.view(-1).view(torch.uint8)
                           if b.dtype != torch.float64 else b)


def test_ppo_loss_head_ls_op(be):
    from ase_amd import ops  # noqa: F401
    M, A, Z = 128, 31, 16
    mu, ls_rows, ls_vec, mb, new_z, value = _head_inputs(M, A, Z, 5, False)
    dev = 'cuda'
    for ls in (ls_rows, ls_vec):
        stats, d_mu, d_ls, d_v = torch.ops.ase_hip.ppo_loss_head_ls(
            mu.to(dev), value.to(dev), mb['actions'].to(dev), mb['mu'].to(dev), mb['sigma'].to(dev), mb['old_logp_actions'].to(dev),
            mb['advantages'].to(dev), mb['old_values'].to(dev), mb['returns'].to(dev), mb['rand_action_mask'].to(dev), ls.to(dev),
            0.2, 5.0, 10.0, False, 0.01)
        s_r, gmu_r, gls_r, gv_r = _reference(mu, ls, mb, new_z, value, M, A, True, False, False, False, 0.2, 5.0, 10.0, 0, 0, 0.01)
        close(stats.cpu(), s_r.float(), 1e-4, 1e-6, 'stats')
        close(d_mu.cpu(), gmu_r.float(), 2e-4, 2e-4 * float(gmu_r.abs().max()), 'd_mu')
        got = d_ls.cpu() if ls.dim() == 2 else d_ls.cpu().sum(0)
        close(got, gls_r.float(), 1e-3, 2e-4 * float(gls_r.abs().max()), 'd_logstd')
        close(d_v.cpu(), gv_r.float(), 2e-4, 1e-6, 'd_value')


# ------------------------------------------------------------------------------------------------ rollout sampling
def test_sample_actions_per_row_logstd(be):
    n, A = 4096, 31
    dev = 'cuda'
    g = torch.Generator().manual_seed(3)
    MU = torch.zeros(n, 128, device=dev)
    MU[:, :A] = torch.randn(n, A, generator=g).to(dev) * 0.5
    MU[:, 64:64 + A] = (-1.5 + 0.5 * torch.randn(n, A, generator=g)).to(dev)
    ls = MU[:, 64:64 + A]
    rng = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    mus, sig, act, nlp = torch.empty(n, A, **f32), torch.empty(n, A, **f32), torch.empty(n, A, **f32), torch.empty(n, 1, **f32)
    be.sample_actions(MU, ls, None, rng, mus, sig, act, nlp, None, n, A, False, logstd_rows=True)
    torch.cuda.synchronize()
    assert torch.equal(mus, MU[:, :A])
    close(sig, torch.exp(ls), 1e-6, 0, 'sigma = exp(logstd) per row')
    ref = 0.5 * (((act - mus) / sig) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * A + ls.sum(-1)
    close(nlp.view(-1), ref, 1e-5, 1e-4, 'neglogp')
    eps = ((act - mus) / sig).cpu()
    assert abs(float(eps.mean())) < 0.01 and abs(float(eps.std()) - 1.0) < 0.01
    # stride 0 is today's broadcast
    sig0 = torch.empty(n, A, **f32)
    be.sample_actions(MU, ls[0].contiguous(), None, rng, mus, sig0, act, nlp, None, n, A, False)
    torch.cuda.synchronize()
    assert torch.equal(sig0, torch.exp(ls[0]).expand(n, A).contiguous())


# ------------------------------------------------------------------------------------------------ agents against the reference
@pytest.mark.parametrize('name', SIGMA_GOLDENS)
def test_two_epochs_learned_sigma_f32(be, name):
    G = _load(name)
    ag = make_agent(G, be, device='cuda', precision='f32')
    captured = {}
    orig = ag.engine.phase_finish

    def grab(*a, **kw):
        r = orig(*a, **kw)
        if not captured:
            torch.cuda.synchronize()
            captured.update({k: v.detach().cpu().clone() for k, v in ag.engine.export_grads().items()})
        return r
    ag.engine.phase_finish = grab
    replay_epochs(G, ag, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25)
    fg, seed = G['epochs'][0]['first_grads'], G.get('sample', {}).get('seed', 0)
    for k in ('sigma', 'sigma.weight', 'sigma.bias'):
        if k in fg:
            close_entry(k, captured[k], fg[k], 3e-4, 1e-6, seed, 'first-step gradient ' + k)


@pytest.mark.parametrize('precision,loss_tol', [('f16gpx3', 2e-3), ('bf16', 2e-2)])
def test_sighead_16bit_losses(be, precision, loss_tol):
    G = _load('ase_sighead_tiny')
    ag = make_agent(G, be, device='cuda', precision=precision)
    infos = replay_epochs(G, ag, rtol=0, wtol=0, check=False)
    scale = {'actor_loss': 1.0, 'enc_loss': 1.0, 'kl': 0.1, 'b_loss': 1.0}
    for i, ref in enumerate(G['epochs'][0]['steps']):
        for k in ('actor_loss', 'critic_loss', 'b_loss', 'disc_loss', 'disc_grad_penalty', 'enc_loss', 'amp_diversity_loss'):
            if k in ref:
                a, b = float(infos[0][k][i]), float(ref[k].mean())
                assert a == a and abs(a - b) <= loss_tol * max(abs(b), scale.get(k, 0.0)), (precision, k, i, a, b)


@pytest.mark.parametrize('name', ['ase_sighead_tiny', 'amp_sighead_tiny', 'ppo_sighead_tiny', 'ase_lsig_tiny'])
def test_rollout_inference_per_row_sigma(be, name):
    """The engine's eval forward on the regenerated first-epoch observations: the reference rollout's per-row mus / sigmas /
    values (E['exp']) at f32."""
    G = regenerate(_load(name))
    ag = make_agent(G, be, device='cuda', precision='f32')
    check_rollout_inference(G, ag, rtol=1e-5, atol=1e-5)
    if name != 'ase_lsig_tiny':
        E = G['epochs'][0]
        H, N = E['exp']['obses'].shape[:2]
        extra = (E['exp']['ase_latents'].reshape(H * N, -1).cuda(),) if G['kind'] == 'ase' else ()
        mu, sg, _ = ag._policy(E['exp']['obses'].reshape(H * N, -1).cuda(), *extra)
        assert float(sg.std(0).max()) > 0        # per-state, not one vector


@pytest.mark.parametrize('name', ['amp_sighead_tiny', 'ppo_sighead_tiny'])
def test_graph_and_eager_learned_sigma(be, name):
    """Captured launch programs and the eager launches give the same trajectory (the cross-step schedule included)."""
    G = _load(name)
    flats = []
    for graph in (False, True):
        ag = make_agent(G, be, device='cuda', precision='f32', graph_capture=graph)
        replay_epochs(G, ag, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25)
        flats.append(ag.model.a2c_network.flat_params.detach().cpu().clone())
    assert torch.allclose(flats[0], flats[1], rtol=1e-5, atol=2e-6)


def test_mixed_precision_epoch_finite(be):
    G = _load('ase_sighead_tiny')
    ag = make_agent(G, be, device='cuda', precision='f16', mixed_precision=True)
    infos = replay_epochs(G, ag, rtol=0, wtol=0, check=False)
    for k, v in infos[0].items():
        if isinstance(v, list) and v and torch.is_tensor(v[0]):
            assert all(bool(torch.isfinite(x.float()).all()) for x in v), k
    assert bool(torch.isfinite(ag.model.a2c_network.flat_params).all())


def _dp_worker(rank, world, port, name, out):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from ase_amd.backend import HipBackend
    G = _load(name)
    ag = make_agent(G, HipBackend('cuda:0'), device='cuda:0', precision='f32', world_size=world, rank=rank)
    replay_epochs(G, ag, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25)
    torch.cuda.synchronize()
    if rank == 0:
        torch.save(ag.model.a2c_network.flat_params.detach().cpu().clone(), out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_vector_form_match_one_rank(be, tmp_path):
    import socket
    import torch.multiprocessing as mp
    G = _load('ase_lsig_tiny')
    ag1 = make_agent(G, be, device='cuda', precision='f32')
    replay_epochs(G, ag1, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'r0.pt')
    mp.spawn(_dp_worker, args=(2, port, 'ase_lsig_tiny', out), nprocs=2, join=True)
    flat = torch.load(out)
    assert torch.allclose(flat, ag1.model.a2c_network.flat_params.detach().cpu(), rtol=1e-5, atol=G['cfg']['learning_rate'] * 0.25)


@pytest.mark.parametrize('name', ['ase_lsig_tiny', 'ppo_sighead_tiny'])
def test_checkpoint_continue_equals_uninterrupted(be, name, tmp_path):
    """Save after one update, restore into a fresh agent: weights and Adam moments (the sigma tensors' included) restored
    exactly; for the PPO agent, whose whole state is in the checkpoint, the next update then equals the uninterrupted one (the
    AMP / ASE agents' replay ring is not part of the reference's checkpoint)."""
    G = _load(name)
    a = make_agent(G, be, device='cuda', precision='f32')
    replay_epochs(G, a, rtol=3e-4, wtol=G['cfg']['learning_rate'] * 0.25)
    w = a.get_full_state_weights()
    torch.save(w, str(tmp_path / 'ck.pt'))
    b = make_agent(G, be, device='cuda', precision='f32')
    b.set_full_state_weights(torch.load(str(tmp_path / 'ck.pt'), weights_only=False))
    ea, eb = a.engine, b.engine
    n = ea.n_train
    assert torch.equal(ea.params[:n], eb.params[:n]) and torch.equal(ea.adam_m[:n], eb.adam_m[:n]) and \
        torch.equal(ea.adam_v[:n], eb.adam_v[:n])
    for k in ('sigma', 'sigma.weight', 'sigma.bias'):
        if k in a.model.a2c_network.param_slices:
            o, shp = a.model.a2c_network.param_slices[k]
            assert float(ea.adam_v[o:o + math.prod(shp)].abs().sum()) > 0, k      # the moments moved and were restored
    if G['kind'] != 'ppo':
        return
    for ag in (a, b):
        replay_epochs(G, ag, rtol=0, wtol=0, check=False)
    torch.cuda.synchronize()
    assert torch.allclose(a.model.a2c_network.flat_params, b.model.a2c_network.flat_params, rtol=1e-6, atol=1e-7)


def test_player_samples_with_per_row_sigma(be):
    G = regenerate(_load('ppo_sighead_tiny'))
    ag = make_agent(G, be, device='cuda', precision='f32')
    E = G['epochs'][0]
    obs = E['exp']['obses'].reshape(-1, G['spec']['obs_size'])[:64].cuda()
    from tests.helpers import set_rms
    set_rms(ag.engine.obs_state, E['rms_before']['obs'])
    rng = torch.tensor([4321, 0], dtype=torch.int64, device='cuda')
    res = ag.engine.policy_act(obs, None, None, rng)
    out = ag.engine.policy_forward(obs, None, want=('mu', 'logstd'))
    torch.cuda.synchronize()
    close(res['sigmas'], torch.exp(out['logstd']), 1e-6, 0, 'player sigma')
