"""engine_opts gp_fuse on the emulator: with the helper launches of the penalty's value path folded into the matrix launches that
produce their inputs (seed, 16-bit copies of the chain, sum of squares) the step computes what the separate launches computed -
the emulator does the same arithmetic in both, so everything is equal but the penalty's f64 sum, which may differ by rounding."""
import os

import pytest
import torch

from ase_amd import lib as L
from ase_amd.engine import UpdateEngine
from tests.emu_backend import EmuBackend
from tests.emu_gp_fuse import FusedEmuBackend
from tests.helpers import build_net, set_rms

PENALTY = ('disc_grad_penalty', 'disc_loss', 'loss')      # scalars that contain the f64 sum


def run_steps(G, be, steps=1, device='cpu', engine_opts=None, between=None, dtype=torch.float16, sync=None, cfg_extra=None):
    """tests/test_engine_emu.first_step with gp_f32 = 'x3' and `steps` steps on the same minibatch; between(net, eng) runs after
    every step but the last (the routes that change the weights behind the engine's back)."""
    kind, cfg, E = G['kind'], dict(G['cfg']), G['epochs'][0]
    cfg['gp_f32'] = 'x3'
    cfg['engine_opts'] = dict(engine_opts or {})
    cfg.update(cfg_extra or {})
    net = build_net(G, device)
    mb = {k: v.to(device) for k, v in E['first_minibatch'].items()}
    M = mb['obs'].shape[0]
    eng = UpdateEngine(kind, net, cfg, be, minibatch=M, amp_minibatch=cfg['amp_minibatch_size'], dtype=dtype)
    set_rms(eng.obs_state, E['rms_step0_before']['obs'])
    set_rms(eng.amp_state, E['rms_step0_before']['amp'])
    idx = torch.arange(M, dtype=torch.int32, device=device)
    streams = [(mb['amp_obs'], idx, (0, 0)), (mb['amp_obs_replay'], idx, (0, 0)), (mb['amp_obs_demo'], idx, (0, 0))]
    z = E['new_zs'][0].to(device) if E['new_zs'] else None
    out = []
    for i in range(steps):
        eng.step(mb, idx, (0, 0), streams, new_z=z)
        if sync:
            sync()
        out.append(snapshot(net, eng))
        if between is not None and i + 1 < steps:
            between(net, eng)
    return net, eng, out


def snapshot(net, eng):
    g = eng._gp32
    return {'res': {k: v.detach().cpu().clone() for k, v in eng.results().items()},
            'grads': {k: v.detach().cpu().clone() for k, v in eng.export_grads().items()},
            'bits': [b.cpu().clone() for b in g.bits],
            'chain16': [x.cpu().clone() for x in eng.Gp] + [eng.G0.cpu().clone()],
            'seed32': g.Gp[-1].cpu().clone(),
            'weights': {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}}


def assert_same_step(on, off, what='', exact=True, lr=0.0):
    """exact=False (two runs on a GPU, whose f32 / f64 atomics add in another order from run to run): losses and gradients within
    1e-5 of the tensor's largest magnitude - a few f32 roundings, 6e-8 each, over the handful of partial sums of a tiny layer -
    and weights within the 5 % of one learning-rate step that the golden first-step checks allow; what the fused epilogues
    write themselves (masks, seed, 16-bit chain) stays bit-equal."""
    def same(a, b, rtol):
        a, b = a.double(), b.double()
        d = float((a - b).abs().max()) if a.numel() else 0.0
        return d <= rtol * float(b.abs().max())

    for k, v in off['res'].items():
        if k in PENALTY or not exact:       # the f64 sum in another order of additions: rounding level of its f32 result
            assert torch.allclose(on['res'][k], v, rtol=1e-6 if exact else 1e-5, atol=0), (what, k, on['res'][k], v)
        else:
            assert torch.equal(on['res'][k], v), (what, k, on['res'][k], v)
    assert set(on['grads']) == set(off['grads'])
    for k, v in off['grads'].items():
        assert torch.equal(on['grads'][k], v) if exact else same(on['grads'][k], v, 1e-5), (what, 'grad', k)
    for a, b in zip(on['bits'], off['bits']):
        assert torch.equal(a, b), (what, 'bits')
    for a, b in zip(on['chain16'], off['chain16']):
        assert torch.equal(a, b), (what, '16-bit chain')
    assert torch.equal(on['seed32'], off['seed32']), (what, 'seed')
    for k, v in off['weights'].items():
        if exact:
            assert torch.equal(on['weights'][k], v), (what, 'weight', k)
        else:
            assert float((on['weights'][k].double() - v.double()).abs().max()) <= 0.05 * lr, (what, 'weight', k)


@pytest.fixture(scope='module')
def G(golden_dir):
    return torch.load(os.path.join(golden_dir, 'ase_tiny.pt'), weights_only=False)


@pytest.fixture(scope='module')
def unfused(G):
    """Two steps of the launch sequence without gp_fuse (computed once, shared, not modified)."""
    be = FusedEmuBackend()
    _, eng, out = run_steps(G, be, steps=2, engine_opts={'gp_fuse': False})
    assert not eng._gp_fuse and be.fused_launches == 0
    return out, (be.helper_launches, be.normalize_launches)


def test_gp_fuse_matches_the_separate_launches(G, unfused):
    off, off_helpers = unfused
    be = FusedEmuBackend()
    _, eng, on = run_steps(G, be, steps=2)                       # 'auto': on, the backend has the capability
    assert eng.gp32 and eng._gp_fuse
    nl = len(eng.disc)
    assert be.fused_launches == 2 * (nl + 1)                     # seed launch, nl - 1 inner chain launches, the last chain launch
    assert off_helpers[0] - be.helper_launches == 2 * 3          # gp_seed, sqnorm and the conversion launch: gone
    if eng.amp % 4 == 0:                                         # ... and the value path's own normalise launch (16-byte rows)
        assert eng._st.gp_x_done and off_helpers[1] - be.normalize_launches == 2
    assert eng._gp_split and be.split_shadow_writes == 2 * nl       # the trunk's half-split shadows: by the optimizer launch
    assert float(on[0]['res']['disc_grad_penalty']) > 0
    assert_same_step(on[0], off[0], 'step 0')
    assert_same_step(on[1], off[1], 'step 1 (post-Adam weights)')


def test_gp_fuse_needs_the_capability(G, unfused):
    """A backend without the capability attribute (tests/emu_backend.py as it is) takes the old sequence whatever the option says."""
    be = EmuBackend()
    be.x3 = False
    _, eng, out = run_steps(G, be, engine_opts={'gp_fuse': True})
    assert eng.gp32 and not eng._gp_fuse
    assert_same_step(out[0], unfused[0][0], 'no capability')


ROUTES = {
    # name: (cfg_extra, engine_opts, what happens between the two steps)
    'refresh_shadows': ({}, {}, 'scale+refresh'),            # bench.py's parity protocol: masters changed, then refresh_shadows()
    'state_dict_load': ({}, {}, 'load'),                     # checkpoint load: load_state_dict, then refresh_shadows() (agents.set_weights)
    'truncate_grads': ({'truncate_grads': True}, {}, None),  # the end-of-step optimizer form (clip -> adam -> refresh_shadows)
    'fused_apply_false': ({}, {'fused_apply': False}, None),  # adam + refresh_shadows instead of the fused launch
    'dyn_scale': ({'loss_scale': 'dynamic', 'loss_scaler': {'init_scale': 256.0, 'backoff_factor': 0.5, 'growth_factor': 2.0,
                                                            'growth_interval': 2000}}, {}, None),      # _dyn_apply
}


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_gp_fuse_shadows_follow_every_route_that_changes_the_weights(G, route):
    """With gp_fuse the value path no longer refreshes its half-split shadows itself: they are current behind the fused optimizer
    launch (apply_multi_split) and behind refresh_shadows, in which every other route ends.  Each route changes the discriminator's
    weights between two steps; the second step's penalty (and everything else) must be the unfused run's, which re-reads the
    masters every step."""
    cfg_extra, opts, action = ROUTES[route]

    def change(net, eng):
        if action == 'scale+refresh':
            with torch.no_grad():
                for d in eng.disc:
                    d.W[0].mul_(1.25)
            eng.refresh_shadows()
        elif action == 'load':
            sd = {k: v.clone() for k, v in net.state_dict().items()}
            for k in sd:
                if '_disc_mlp' in k and k.endswith('weight'):
                    sd[k] = sd[k] * 1.25
            net.load_state_dict(sd)
            eng.refresh_shadows()

    res = {}
    for fuse in (True, False):
        be = FusedEmuBackend()
        _, eng, out = run_steps(G, be, steps=2, engine_opts=dict(opts, gp_fuse=fuse), between=change, cfg_extra=cfg_extra)
        assert eng._gp_fuse == fuse and eng.dyn_scale == (route == 'dyn_scale') and eng.truncate == (route == 'truncate_grads')
        if fuse:
            # no refresh of its own in the value path: split writes by the optimizer launch, or refresh_shadows behind the route
            assert eng._gp_split == (route != 'fused_apply_false')
            assert (be.split_shadow_writes > 0) == (route not in ('truncate_grads', 'fused_apply_false'))
        res[fuse] = out
    assert float(res[False][1]['res']['disc_grad_penalty']) > 0
    assert_same_step(res[True][1], res[False][1], route)
    assert not torch.equal(res[True][1]['res']['disc_grad_penalty'], res[True][0]['res']['disc_grad_penalty'])

