"""engine_opts gp_stack on against off: the backward of the penalty chain below its top layer rides on the loss rows' forward
(ase_hip_gemm_nt_stacked), the value path's last launch moves into the branch's head with a sum-of-squares cell of its own and the
discriminator's loss head folds that cell into the step's accumulator."""
import copy
import os

import pytest
import torch

from ase_amd import lib as L
from tests.test_gp_fuse_emu import assert_same_step, run_steps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('capture', [None, 'hipgraph'])
def test_engine_gp_stack_on_against_off(capture, golden_dir):
    """The tiny fixture in f16 storage with gp_f32 = 'x3', multi-stream, the value path inline (gp_stream off), two steps: gp_stack
    on computes what off computes, under the bounds of test_engine_gp_fuse_on_against_off (two GPU runs add their atomics in
    another order).  At this size the library runs every stacked launch as its two plain launches, so what the test pins is the
    SCHEDULE: the whole value path in the branch's head - under the cross-step schedule (capture None) in front of begin_step -
    the private cell, zeroed with the amp sums, and its fold by the loss head.  capture = 'hipgraph': the schedule a captured
    graph needs (serial prologue, no cross-step head), nothing is captured here."""
    from ase_amd.backend import HipBackend
    G = torch.load(os.path.join(golden_dir, 'ase_tiny.pt'), weights_only=False)
    out = {}
    for stack in (False, True):
        _, eng, out[stack] = run_steps(G, HipBackend(), steps=2, device='cuda', sync=torch.cuda.synchronize,
                                       engine_opts={'gp_stack': stack, 'gp_stream': False},
                                       cfg_extra={'graph_capture': capture} if capture else None)
        assert eng.multi_stream and eng._gp_fuse and not eng._gp_side and eng._gp_stack == stack and eng._stacked() == stack
        assert eng._xstep == (capture is None)
        assert eng.gp_sq.numel() == int(stack)
    lr = float(G['cfg']['learning_rate'])
    for i in (0, 1):
        on, off = float(out[True][i]['res']['disc_grad_penalty']), float(out[False][i]['res']['disc_grad_penalty'])
        print(f'step {i}: disc_grad_penalty stacked {on!r} unstacked {off!r}')
        # (the bound test_last_chain_launch_twin_only_and_sum_of_squares holds the same sum to: f64 atomics in another order)
        assert on > 0 and abs(on - off) <= 1e-6 * abs(off), (i, on, off)
        assert_same_step(out[True][i], out[False][i], f'step {i}', exact=False, lr=lr)


def _ulp_diff(a, b):
    """Largest distance of two f16 tensors in units of the last place (monotone integer image of the patterns)."""
    def key(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return int((key(a) - key(b)).abs().max())


def test_full_size_step_stacked_against_unstacked():
    """One step at BASELINE config 2's size (minibatch 16384, AMB = 4096, discriminator 1400 -> 1024 -> 1024 -> 512; f16 storage,
    gp_f32 = 'x3', synthetic inputs as tests/test_gpu_engine.py builds them): here the stacked launches of layers 0 and 1 are ONE
    launch of the phased 256 x 256 kernel over 16384 rows, where the unstacked step runs the 192 x 256 phased kernel on the 12288
    loss rows and a generic 64 x 128 tile on the 4096 chain rows.  All three add the products of a K-tile in the same order (k
    ascending, one f32 accumulator per output), so the loss rows' H_l and the chain's dJ/dU_l must be the unstacked run's bit for
    bit (reference side: the UNSTACKED run)."""
    from ase_amd import cfg as defaults
    from ase_amd.backend import HipBackend
    from ase_amd.engine import UpdateEngine
    from ase_amd.learning.network_builder import ASEBuilder
    M, AMB = 16384, 4096
    net_p, cfg0 = defaults.get('ase')
    g = torch.Generator().manual_seed(1)
    z = torch.randn(M, 64, generator=g)
    nz = torch.randn(M, 64, generator=g)
    mb = {'obs': torch.randn(M, 253, generator=g) * 1.5 + 0.2, 'actions': torch.randn(M, 31, generator=g) * 0.1,
          'mu': torch.randn(M, 31, generator=g) * 0.05, 'sigma': torch.full((M, 31), 0.055023),
          'old_logp_actions': torch.randn(M, generator=g),
          'advantages': torch.randn(M, generator=g), 'old_values': torch.randn(M, 1, generator=g),
          'returns': torch.randn(M, 1, generator=g), 'rand_action_mask': (torch.rand(M, generator=g) < 0.8).float(),
          'ase_latents': z / z.norm(dim=-1, keepdim=True), 'amp_obs': torch.randn(M, 1400, generator=g),
          'amp_obs_replay': torch.randn(M, 1400, generator=g) * 1.1, 'amp_obs_demo': torch.randn(M, 1400, generator=g) + 0.3}
    mbg = {k: v.cuda() for k, v in mb.items()}
    nz = (nz / nz.norm(dim=-1, keepdim=True)).cuda()
    idx = torch.arange(M, dtype=torch.int32, device='cuda')
    streams = [(mbg['amp_obs'], idx, (0, 0)), (mbg['amp_obs_replay'], idx, (0, 0)), (mbg['amp_obs_demo'], idx, (0, 0))]
    got = {}
    for stack in (False, True):
        cfg = copy.deepcopy(cfg0)
        cfg.update(minibatch_size=M, amp_minibatch_size=AMB, gp_f32='x3', engine_opts={'gp_stack': stack, 'gp_stream': False})
        torch.manual_seed(0)
        b = ASEBuilder()
        b.load(net_p)
        net = b.build('ase', actions_num=31, input_shape=(253,), num_seqs=1, value_size=1, amp_input_shape=(1400,),
                      ase_latent_shape=(64,), device='cuda')
        be = HipBackend()
        eng = UpdateEngine('ase', net, cfg, be, minibatch=M, amp_minibatch=AMB, dtype=torch.float16)
        assert eng._gp_fuse and eng._stacked() == stack and len(eng.disc) == 3
        d0, d1 = eng.disc[0], eng.disc[1]
        assert be.lib.ase_hip_gemm_nt_kernel_id(4 * AMB, d0.n_pad, d0.k_pad, L.F16) == 2
        assert be.lib.ase_hip_gemm_nt_kernel_id(4 * AMB, d1.n_pad, d1.k_pad, L.F16) == 2
        eng.step(mbg, idx, (0, 0), streams, new_z=nz, apply=False)
        torch.cuda.synchronize()
        got[stack] = {'Hd4': [h.clone() for h in eng.Hd4[:2]], 'G0': eng.G0.clone(), 'top': eng.GpTop.clone(),
                      'bits': [eng._mask_of(h).clone() for h in eng.Hd[:2]],
                      'gp': float(eng.results()['disc_grad_penalty']),
                      'grads': {k: v.clone() for k, v in eng.export_grads().items() if 'disc' in k}}
        del eng, net
    on, off = got[True], got[False]
    assert torch.equal(on['G0'].view(torch.int16), off['G0'].view(torch.int16)) and float(off['G0'].abs().max()) > 0
    Rd = 3 * AMB
    for l in range(2):
        a, r = on['Hd4'][l], off['Hd4'][l]
        print(f'layer {l}: H_l max ulp diff {_ulp_diff(a[:Rd], r[:Rd])}, dJ/dU_l max ulp diff {_ulp_diff(a[Rd:], r[Rd:])}')
        assert float(r[Rd:].abs().max()) > 0 and float((r[Rd:] == 0).float().mean()) > 0.1      # the chain is there, and masked
        assert torch.equal(a[:Rd].view(torch.int16), r[:Rd].view(torch.int16)), f'H_{l}'
        assert torch.equal(a[Rd:].view(torch.int16), r[Rd:].view(torch.int16)), f'dJ/dU_{l}'
        assert torch.equal(on['bits'][l], off['bits'][l]), f'mask bits of H_{l}'
    assert torch.equal(on['top'], off['top'])
    print('disc_grad_penalty stacked', repr(on['gp']), 'unstacked', repr(off['gp']))
    assert on['gp'] > 0 and abs(on['gp'] - off['gp']) <= 1e-6 * abs(off['gp'])
    assert len(off['grads']) > 0
    for k, v in off['grads'].items():           # (f32 atomics of the weight-gradient reduction in another order)
        assert float((on['grads'][k] - v).abs().max()) <= 1e-5 * float(v.abs().max()), k
