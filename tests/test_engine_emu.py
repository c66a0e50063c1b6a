"""Host logic of the update engine (buffer layout, launch sequence, analytic backward incl. the
gradient-penalty chain, concat-column maps, Adam, running statistics) checked on CPU: the engine
drives tests/emu_backend.py (same op semantics as the HIP kernels) and must reproduce what the
REFERENCE produced for the same minibatch (golden vectors): every loss scalar, every gradient
tensor of the first step and the post-Adam weights."""
import copy
import os

import pytest
import torch

from ase_amd.engine import UpdateEngine, _StepState
from tests.emu_backend import EmuBackend
from tests.helpers import build_net, close, get_rms, set_rms

CASES = ['ase_tiny', 'amp_tiny', 'ppo_tiny', 'ase_sep_tiny', 'ase_gp_tiny', 'ase_sep_gp_tiny',
         'ase_swish_tiny']       # swish (SiLU) in the policy MLPs, the discriminator and the encoder: the curved gradient penalty


def build_engine(G, be, dtype, device='cpu', grad_scale=None, engine_opts=None, gp_f32=False):
    """(net, engine, arguments of engine.step for the golden's first minibatch)."""
    kind, cfg, E = G['kind'], dict(G['cfg']), G['epochs'][0]
    if engine_opts:
        cfg['engine_opts'] = engine_opts
    if gp_f32:
        cfg['gp_f32'] = True
    net = build_net(G, device)
    mb = {k: v.to(device) for k, v in E['first_minibatch'].items()}
    M = mb['obs'].shape[0]
    amb = cfg.get('amp_minibatch_size', 0) if kind != 'ppo' else 0
    eng = UpdateEngine(kind, net, cfg, be, minibatch=M, amp_minibatch=amb, dtype=dtype, grad_scale=grad_scale)
    set_rms(eng.obs_state, E['rms_step0_before']['obs'])
    if kind != 'ppo':
        set_rms(eng.amp_state, E['rms_step0_before']['amp'])
    idx = torch.arange(M, dtype=torch.int32, device=device)
    streams = None
    if kind != 'ppo':
        streams = [(mb['amp_obs'], idx, (0, 0)), (mb['amp_obs_replay'], idx, (0, 0)), (mb['amp_obs_demo'], idx, (0, 0))]
    z = E['new_zs'][0].to(device) if E['new_zs'] else None
    return net, eng, ((mb, idx, (0, 0), streams), dict(new_z=z))


def first_step(G, be, dtype, **kw):
    net, eng, (args, kwargs) = build_engine(G, be, dtype, **kw)
    eng.step(*args, **kwargs)
    return net, eng


SCALARS = ['entropy', 'b_loss', 'actor_loss', 'actor_clip_frac', 'kl', 'disc_loss', 'disc_grad_penalty',
           'disc_logit_loss', 'disc_agent_acc', 'disc_demo_acc', 'enc_loss', 'enc_grad_penalty', 'amp_diversity_loss']


def check_first_step(G, net, eng, rtol, gtol, wtol):
    E = G['epochs'][0]
    res, ref = eng.results(), E['steps'][0]
    for k in SCALARS:
        if k in ref:
            close(res[k], ref[k], rtol, rtol * 0.1, k)
    close(res['critic_loss'], ref['critic_loss'].mean(), rtol, 1e-6, 'critic_loss')
    for k in ('disc_agent_logit', 'disc_demo_logit'):
        if k in ref:
            close(res[k], ref[k], rtol * 10, rtol, k)
    grads = eng.export_grads()
    assert set(grads) == set(E['first_grads'])
    for k, g in E['first_grads'].items():
        close(grads[k], g, gtol, gtol * float(g.abs().max()) + 1e-12, 'grad ' + k)
    sd = net.state_dict()
    for k, w in E['sd_after_step0'].items():
        close(sd[k], w, 1e-6, wtol, 'weight ' + k)
    close(get_rms(eng.obs_state)['mean'], E['rms_after']['obs']['mean'] * 0 + get_rms(eng.obs_state)['mean'], 0, 0)


@pytest.mark.parametrize('name', CASES)
def test_first_step_f32_emulated(name, golden_dir):
    G = torch.load(os.path.join(golden_dir, name + '.pt'), weights_only=False)
    net, eng = first_step(G, EmuBackend(), torch.float32)
    lr = G['cfg']['learning_rate']
    check_first_step(G, net, eng, rtol=2e-5, gtol=2e-4, wtol=lr * 0.05)


@pytest.mark.parametrize('name', CASES)
def test_gradient_scale_is_transparent(name, golden_dir):
    """The static gradient scale of half storage (engine.gs; the GradScaler's place, learning/ase_agent.py:216,271-288): the
    loss heads store S * gradient, the data-gradient chains and both gradient-penalty chains carry S, the weight-gradient
    launches and the bias gradients undo it.  With f32 storage a power-of-two S changes nothing but exponents: the golden
    step of the reference is reproduced at the same tolerances with S = 4096 (every net kind, both penalty variants)."""
    G = torch.load(os.path.join(golden_dir, name + '.pt'), weights_only=False)
    net, eng = first_step(G, EmuBackend(), torch.float32, grad_scale=4096.0)
    assert eng.gs == 4096.0
    check_first_step(G, net, eng, rtol=2e-5, gtol=2e-4, wtol=G['cfg']['learning_rate'] * 0.05)


@pytest.mark.parametrize('name', ['ase_tiny', 'amp_tiny', 'ppo_tiny', 'ase_gp_tiny'])
def test_first_step_f16_emulated(name, golden_dir):
    """Half storage (the reference's mixed_precision arithmetic): 11 significant bits on activations, shadow weights and
    back-propagated gradients, f32 accumulation.  On the stress minibatches of the goldens (clip fraction 0.93): losses
    within 1e-2 of the reference, every gradient tensor within 6 % relative L2 (bf16: 8e-2 / 30 %)."""
    G = torch.load(os.path.join(golden_dir, name + '.pt'), weights_only=False)
    net, eng = first_step(G, EmuBackend(), torch.float16)
    assert eng.gs > 1.0
    E = G['epochs'][0]
    res, ref = eng.results(), E['steps'][0]
    for k in ('actor_loss', 'b_loss', 'disc_loss', 'disc_grad_penalty', 'enc_loss', 'amp_diversity_loss', 'kl', 'enc_grad_penalty'):
        if k in ref:
            close(res[k], ref[k], 1e-2, 3e-3, k)
    grads = eng.export_grads()
    for k, g in E['first_grads'].items():
        rel = float((grads[k].double() - g.double()).norm() / (g.double().norm() + 1e-30))
        assert rel < 0.06, ('grad ' + k, rel)


@pytest.mark.parametrize('name', CASES)
def test_deferred_weight_gradients(name, golden_dir):
    """The grouped weight-gradient launches (all layers of a branch queued during its backward, ONE launch per branch
    group - discriminator | policy - at the end of the branch) read nothing the data-gradient chain overwrites: same
    golden result with every layer deferred."""
    G = torch.load(os.path.join(golden_dir, name + '.pt'), weights_only=False)
    be = EmuBackend(group_all=True)
    net, eng = first_step(G, be, torch.float32)
    # discriminator branch | actor + critic + style MLP as the last launch of the step
    assert be.grouped_launches == {'ppo': 1, 'amp': 2, 'ase': 2}[G['kind']] and not eng._tn_queue
    lr = G['cfg']['learning_rate']
    check_first_step(G, net, eng, rtol=2e-5, gtol=2e-4, wtol=lr * 0.05)


def check_truncate_grads(G, be, device='cpu'):
    """The step with the global-norm clip against the reference's golden gradients -> torch.nn.utils.clip_grad_norm_ (restated,
    and checked against torch's own) -> Adam: gradients after the clip and post-Adam weights.  grad_norm is set to half the
    actual norm so that the clip is active.  Shared by the emulator test below and the GPU test (tests/test_gpu_engine.py)."""
    import copy
    from oracle import restated as R
    G = copy.deepcopy(G)
    E = G['epochs'][0]
    total0 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in E['first_grads'].values())))
    G['cfg'].update(truncate_grads=True, grad_norm=0.5 * total0)
    net, eng = first_step(G, be, torch.float32, device=device)
    assert eng.truncate
    grads = {k: v.detach().cpu() for k, v in eng.export_grads().items()}
    tot = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    assert abs(tot - 0.5 * total0) <= 1e-4 * total0                       # clipped to grad_norm
    for k, g in E['first_grads'].items():
        close(grads[k], g * 0.5, 2e-4, 2e-4 * float(g.abs().max()) + 1e-12, 'clipped grad ' + k)
    # oracle: reference gradients -> clip -> Adam
    sd = {k: (v.clone().requires_grad_(k in G['trainable'])) for k, v in G['init_sd'].items()}
    for k, g in E['first_grads'].items():
        sd[k].grad = g.clone()
    tn = R.clip_grad_norm(sd, 0.5 * total0)
    assert abs(float(tn) - total0) <= 1e-5 * total0
    # the restatement against torch's own clip_grad_norm_ on the same gradients
    ps = [torch.nn.Parameter(G['init_sd'][k].clone()) for k in E['first_grads']]
    for p_, g in zip(ps, E['first_grads'].values()):
        p_.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(ps, 0.5 * total0)
    for p_, k in zip(ps, E['first_grads']):
        assert torch.allclose(p_.grad, sd[k].grad, rtol=1e-6, atol=0)
    R.adam_step(sd, R.adam_new(), G['cfg']['learning_rate'])
    got = net.state_dict()
    for k in G['trainable']:
        close(got[k].detach().cpu(), sd[k].detach(), 1e-6, G['cfg']['learning_rate'] * 0.05, 'weight ' + k)
    # and the reported scalars are those of the unclipped step (the clip touches gradients only)
    res, ref = eng.results(), E['steps'][0]
    for k in SCALARS:
        if k in ref:
            close(res[k], ref[k], 1e-4, 1e-5, k)


@pytest.mark.parametrize('name', ['ase_tiny', 'ppo_tiny'])
def test_truncate_grads_matches_clip_grad_norm(name, golden_dir):
    """truncate_grads (learning/ase_agent.py:273-288) on the emulator: see check_truncate_grads."""
    G = torch.load(os.path.join(golden_dir, name + '.pt'), weights_only=False)
    check_truncate_grads(G, EmuBackend())


@pytest.mark.parametrize('name', ['ase_tiny', 'amp_tiny', 'ase_sep_tiny'])
def test_gradient_penalty_in_f32_inside_a_half_engine(name, golden_dir):
    """config gp_f32 (precision 'f16gp32'): the penalty's demo-row path runs in exact f32 with its own forward, chain and
    weight-gradient launches - the reported penalty matches the reference as the f32 engine does, the other scalars stay at
    half's accuracy, and the discriminator trunk's gradients are at least as close to the reference as plain f16's."""
    G = torch.load(os.path.join(golden_dir, name + '.pt'), weights_only=False)
    ref = G['epochs'][0]['steps'][0]
    _, e16 = first_step(G, EmuBackend(), torch.float16)
    _, e32 = first_step(G, EmuBackend(), torch.float16, gp_f32=True)
    r16, r32 = e16.results(), e32.results()
    gp = float(ref['disc_grad_penalty'])
    assert abs(float(r32['disc_grad_penalty']) - gp) <= 2e-6 * abs(gp), (float(r32['disc_grad_penalty']), gp)
    for k in ('actor_loss', 'kl', 'critic_loss'):
        assert abs(float(r32[k].mean()) - float(r16[k].mean())) <= 1e-6 * max(1.0, abs(float(r16[k].mean()))), k    # nothing else moved
    if 'disc_loss' in ref:           # (the discriminator loss contains the penalty: it can only get closer)
        assert abs(float(r32['disc_loss']) - float(ref['disc_loss'])) <= abs(float(r16['disc_loss']) - float(ref['disc_loss'])) + 1e-6
    g16, g32, gref = e16.export_grads(), e32.export_grads(), G['epochs'][0]['first_grads']
    for k, g in gref.items():
        if '_disc_mlp' in k and k.endswith('weight'):
            e_16 = float((g16[k] - g).norm() / g.norm())
            e_32 = float((g32[k] - g).norm() / g.norm())
            assert e_32 <= e_16 * 1.05 + 1e-6, (k, e_16, e_32)


def test_hipgraph_mode_runs_the_plain_schedule(golden_dir):
    """graph_capture: 'hipgraph' switches off what torch's capture cannot hold at config-2 size on ROCm 7.2 (profiles/r06_hipgraph_triage.txt:
    capture_end segfaults on a step whose prologue is forked onto the side streams, and on a fork from a forked stream): the cross-step
    schedule, the short prologue, the penalty value path's own stream - whatever engine_opts asks for; the launch-program mode keeps all."""
    G = torch.load(os.path.join(golden_dir, 'ase_tiny.pt'), weights_only=False)
    for mode, plain in (('hipgraph', True), (True, False)):
        Gm = copy.deepcopy(G)
        Gm['cfg'].update(graph_capture=mode, engine_opts={'xstep': True, 'short_prologue': True, 'gp_stream': True})
        _, eng = first_step(Gm, EmuBackend(), torch.float32)
        assert (eng._xstep, eng._short_prologue, eng._gp_side) == ((False, False, False) if plain else (True, True, True)), mode


RETIRED_OPTS = {'style_side': 0, 'style_wg': 0, 'disc_after_style': False, 'style_early': False, 'stream_offset': 0,
                'side_streams': 2, 'tn_early': False, 'gp_value_late': False, 'gp_split': 'f16', 'gp_scale_split': True}


@pytest.mark.parametrize('name', sorted(RETIRED_OPTS))
def test_retired_engine_opts_are_unknown(name, golden_dir):
    """The schedule options that lost their A/B are gone with the paths they selected: passing one, even with
    its old default, is refused like any other unknown key."""
    G = torch.load(os.path.join(golden_dir, 'ase_tiny.pt'), weights_only=False)
    with pytest.raises(AssertionError, match='unknown engine_opts'):
        first_step(G, EmuBackend(), torch.float32, engine_opts={name: RETIRED_OPTS[name]})


# the fields of engine._StepState; each was an engine attribute of the same name behind an underscore
STEP_STATE_FIELDS = ['disc_fwd_out', 'stats_exchanged', 'merged_stats', 'stats_mark_a', 'stats_mark_b', 'pre_done', 'prep', 'lat_ready',
                     'fill_done', 'early_fork', 'enc_z_ready', 'gp_x_done', 'gp_value_done', 'disc_acc_mark', 'acc_in_bucket', 'lr_live']


def test_step_state_is_replaced_every_step(golden_dir):
    """What the phases of a step hand each other lives in ONE object (engine._StepState), which phase_stats replaces at the top of
    every step; none of the sixteen loose attributes it replaced is left on the engine."""
    G = torch.load(os.path.join(golden_dir, 'ase_tiny.pt'), weights_only=False)
    net, eng, (args, kwargs) = build_engine(G, EmuBackend(), torch.float32)
    seen = [eng._st]
    for _ in range(2):
        eng.step(*args, **kwargs)
        seen.append(eng._st)
    assert all(type(st) is _StepState for st in seen)
    assert seen[2] is not seen[1] and seen[1] is not seen[0]
    assert sorted(_StepState.__slots__) == sorted(STEP_STATE_FIELDS) and len(STEP_STATE_FIELDS) == 16
    for name in STEP_STATE_FIELDS:
        assert not hasattr(eng, '_' + name), name


def test_step_state_refuses_unknown_fields(golden_dir):
    """__slots__: a misspelled field raises instead of creating an attribute nobody reads."""
    G = torch.load(os.path.join(golden_dir, 'ppo_tiny.pt'), weights_only=False)
    _, eng = first_step(G, EmuBackend(), torch.float32)
    with pytest.raises(AttributeError):
        eng._st.lat_redy = None
    with pytest.raises(AttributeError):
        _StepState().disc_acc_mrak = None


def test_step_state_disc_acc_mark_stays_none_without_discriminator(golden_dir):
    """Kind 'ppo' has no discriminator branch: nothing sets its mark, and a fresh state per step means no earlier one survives."""
    G = torch.load(os.path.join(golden_dir, 'ppo_tiny.pt'), weights_only=False)
    _, eng = first_step(G, EmuBackend(), torch.float32)
    assert eng._st.disc_acc_mark is None
