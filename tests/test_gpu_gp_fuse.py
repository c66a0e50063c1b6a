"""The fused epilogue duties of the half-split f32 NT launches (ase_hip_gemm_nt_ex: seed, 16-bit twin, sum of squares) against
the launch sequence they replace on the same device - the plain launch, then ase_hip_gp_seed / the conversion launch of
ase_hip_gather_multi / ase_hip_sqnorm - and the engine with engine_opts gp_fuse on against off."""
import os

import pytest
import torch

from ase_amd import lib as L
from tests import ref_split_pack as S
from tests.test_gp_fuse_emu import assert_same_step, run_steps

pytestmark = pytest.mark.gpu

EA, EB = 12, 11                    # operand exponents of the value path's chain launches (engine._gp_value)
# (M, N, K) -> kernel: the two f32h_t instantiations the six launches of config 2 run (4: 64 x 128 tile, 5: 64 x 64 tile), each at
# the smallest grid that selects it, and one ragged shape (M no multiple of 64, N = 32 x 5: half a wave tile past the last full one)
SHAPES = [((4096, 1024, 64), 4), ((64, 128, 32), 5), ((200, 160, 96), 5),
          # ... and the fused instantiations of the other tiles, which the value path takes at other widths / row counts: the narrow-
          # output tile (0), the 128 x 128 tile with 128- and 64-byte staged rows (1), the 256 x 256 tile with both (3)
          ((64, 64, 16), 0), ((4096, 2048, 32), 1), ((64, 128, 16), 1), ((12288, 1024, 32), 3), ((12288, 1024, 16), 3)]


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(x3='f16')


def _operands(be, M, N, K, seed, a_scale):
    """A as the engine's operands are (|x| <= 5 for inputs, O(1e-2) chain values), weights ~ N(0, 0.03^2) as pre-split shadows."""
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) * a_scale).clamp_(-5, 5).cuda()
    W = (torch.randn(N, K, generator=g) * 0.03).cuda()
    Ws, Wts = torch.zeros(N, K, device='cuda'), torch.zeros(K, N, device='cuda')
    be.refresh_shadow(W, Ws, Wts, K, K, x3_exp=EB)
    return A, Ws


def _convert(be, src, dst, M):
    code = {torch.float16: L.F16, torch.bfloat16: L.BF16}[dst.dtype]
    desc = torch.tensor([[src.data_ptr(), src.stride(0), src.shape[1], dst.data_ptr(), dst.stride(0), code]], dtype=torch.int64,
                        device='cuda')
    be.gather_multi(desc, [(src, src.shape[1], dst)], None, (0, 0), M)


def _bits(mask_words, N):
    return ((mask_words.to(torch.int64).unsqueeze(-1) >> torch.arange(32, device=mask_words.device)) & 1).reshape(mask_words.shape[0], -1)[:, :N]


@pytest.mark.parametrize('shape,kid', SHAPES)
def test_seed_launch(be, shape, kid):
    """Last forward layer: bias + ReLU + mask_out, the seed s w[n] [h > 0] instead of h, f32 and f16."""
    M, N, K = shape
    assert be.lib.ase_hip_gemm_nt_kernel_id(M, N, K, L.F32H3) == kid
    A, Ws = _operands(be, M, N, K, 1, 2.5)
    g = torch.Generator().manual_seed(2)
    bias = (torch.randn(N, generator=g) * 0.05).cuda()
    width = N - 3                                     # logit weights of the real columns only; the padding columns store 0
    w = torch.randn(width, generator=g).cuda()
    s = 0.0173
    kw = dict(bias=bias, act=L.ACT_RELU, x3_exps=(EA, EB))
    # today's sequence
    H, m0 = torch.zeros(M, N, device='cuda'), torch.zeros(M, N // 32, dtype=torch.int32, device='cuda')
    G0, T0 = torch.zeros(M, N, device='cuda'), torch.zeros(M, N, dtype=torch.float16, device='cuda')
    be.gemm_nt(A, Ws, H, M, N, K, mask_out=m0, **kw)
    be.gp_seed(H, w, G0, M, width, scale=s)
    _convert(be, G0, T0, M)
    # fused
    G1, m1 = torch.full((M, N), 7.0, device='cuda'), torch.zeros(M, N // 32, dtype=torch.int32, device='cuda')
    T1 = torch.full((M, N), 7.0, dtype=torch.float16, device='cuda')
    be.gemm_nt(A, Ws, G1, M, N, K, mask_out=m1, seed=(w, s), twin=T1, **kw)
    torch.cuda.synchronize()
    assert 0.2 < float((H > 0).float().mean()) < 0.8
    assert torch.equal(m1, m0)
    assert torch.equal(_bits(m1, N).bool(), H > 0)
    assert torch.equal(G1.view(torch.int32), G0.view(torch.int32))          # bits: -0 where a negative weight meets a closed unit
    assert torch.equal(T1.view(torch.int16), T0.view(torch.int16))


@pytest.mark.parametrize('shape,kid', SHAPES)
def test_chain_launch_with_twin(be, shape, kid):
    """Inner chain launch: bit-mask operand, f32 output and its bf16 twin."""
    M, N, K = shape
    assert be.lib.ase_hip_gemm_nt_kernel_id(M, N, K, L.F32H3) == kid
    A, Ws = _operands(be, M, N, K, 3, 0.02)
    g = torch.Generator().manual_seed(4)
    mask = torch.randint(-2 ** 31, 2 ** 31, (M, N // 32), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    kw = dict(aux=mask, aux_mode=L.AUX_RELU_BITS, x3_exps=(EA, EB))
    C0, T0 = torch.zeros(M, N, device='cuda'), torch.zeros(M, N, dtype=torch.bfloat16, device='cuda')
    be.gemm_nt(A, Ws, C0, M, N, K, **kw)
    _convert(be, C0, T0, M)
    C1, T1 = torch.full((M, N), 7.0, device='cuda'), torch.full((M, N), 7.0, dtype=torch.bfloat16, device='cuda')
    be.gemm_nt(A, Ws, C1, M, N, K, twin=T1, **kw)
    torch.cuda.synchronize()
    assert float(C0.abs().max()) > 0
    assert torch.equal((C0 != 0), _bits(mask, N).bool() & (C0 != 0))
    assert torch.equal(C1.view(torch.int32), C0.view(torch.int32))
    assert torch.equal(T1.view(torch.int16), T0.view(torch.int16))


@pytest.mark.parametrize('shape,kid', SHAPES)
def test_last_chain_launch_twin_only_and_sum_of_squares(be, shape, kid):
    """Last chain launch: alpha = S, no f32 store (the f32 buffer stays untouched), f16 twin, scale * factor * sum of squares.
    Sum of squares: each f32 partial over 4 squares carries at most 4 * 2^-24 relative, everything behind it is f64 - the fused
    launch, ase_hip_sqnorm and the f64 sum of the stored values agree within 1e-6 relative."""
    M, N, K = shape
    A, Ws = _operands(be, M, N, K, 5, 0.02)
    S, scale = 1024.0, 3.0e-3
    dyn = torch.tensor([0.5, 0.0], device='cuda')                             # scale record {factor, overflow count}
    kw = dict(alpha=S, x3_exps=(EA, EB))
    C0, T0 = torch.zeros(M, N, device='cuda'), torch.zeros(M, N, dtype=torch.float16, device='cuda')
    acc0 = torch.zeros(4, dtype=torch.float64, device='cuda')
    be.gemm_nt(A, Ws, C0, M, N, K, **kw)
    be.sqnorm(C0, M, N, acc0, 2, scale=scale, dyn=dyn)
    _convert(be, C0, T0, M)
    C1, T1 = torch.full((M, N), 7.0, device='cuda'), torch.full((M, N), 7.0, dtype=torch.float16, device='cuda')
    acc1 = torch.zeros(4, dtype=torch.float64, device='cuda')
    be.gemm_nt(A, Ws, C1, M, N, K, twin=T1, store=False, sq=(acc1, 2, scale, dyn), **kw)
    # ... and with the f32 store
    C2, acc2 = torch.full((M, N), 7.0, device='cuda'), torch.zeros(4, dtype=torch.float64, device='cuda')
    be.gemm_nt(A, Ws, C2, M, N, K, sq=(acc2, 2, scale, dyn), **kw)
    torch.cuda.synchronize()
    assert torch.equal(C1, torch.full_like(C1, 7.0))
    assert torch.equal(T1.view(torch.int16), T0.view(torch.int16))
    assert torch.equal(C2.view(torch.int32), C0.view(torch.int32))
    ref = scale * 0.5 * float((C0.double() ** 2).sum())
    got0, got1, got2 = float(acc0[2]), float(acc1[2]), float(acc2[2])
    print('sum of squares: f64 torch %.12e  sqnorm %.12e  fused %.12e / %.12e' % (ref, got0, got1, got2))
    assert ref > 0 and float(dyn[1]) == 0
    for got in (got1, got2):
        assert abs(got - got0) <= 1e-6 * abs(got0) and abs(got - ref) <= 1e-6 * abs(ref), (got, got0, ref)
    assert float(acc1[[0, 1, 3]].abs().sum()) == 0


def test_fused_duties_are_refused_outside_the_half_split(be):
    """A missing kernel is an error: other storage types have no fused epilogue."""
    A, B, Cm = torch.zeros(64, 32, device='cuda'), torch.zeros(128, 32, device='cuda'), torch.zeros(64, 128, device='cuda')
    T = torch.zeros(64, 128, dtype=torch.float16, device='cuda')
    rc = be.lib.ase_hip_gemm_nt_ex(A.data_ptr(), 32, B.data_ptr(), 32, Cm.data_ptr(), 128, None, None, 0, 0, 0, None, 0, None, 0,
                                   64, 128, 32, L.ACT_NONE, L.AUX_NONE, 0, 1.0, None, L.F32, None, 0, 0.0, T.data_ptr(), 128, L.F16,
                                   None, 0.0, None, None)
    assert rc == -1 and b'gemm_nt_ex' in be.lib.ase_hip_last_error()


def _apply_case(n, k, split_src, gap, wide):
    """One layer through ase_hip_apply_multi_v2 (Adam step + 16-bit shadows + the half-split pair) -> the pair it wrote and the pair
    ase_hip_refresh_shadow(x3_exp = 11) writes from the UPDATED masters."""
    import struct
    from ase_amd.backend import HipBackend
    be = HipBackend()
    g = torch.Generator().manual_seed(7)
    kp, npad = (k + gap + 31) // 32 * 32, (n + 31) // 32 * 32
    dev = 'cuda'
    W = (torch.randn(n, k, generator=g) * 0.03).to(dev)
    b = torch.zeros(n, device=dev)
    gW, mW, vW = (torch.randn(n, k, generator=g) * 1e-3).to(dev), torch.zeros(n, k, device=dev), torch.zeros(n, k, device=dev)
    gb, mb, vb, bs = (torch.zeros(n, device=dev) for _ in range(4))
    ws, wts = torch.zeros(n, kp, dtype=torch.float16, device=dev), torch.zeros(kp, npad, dtype=torch.float16, device=dev)
    Ws3, Wts3, R3, Rt3 = (torch.full((n, kp), S.SENTINEL, device=dev), torch.full((kp, npad), S.SENTINEL, device=dev),
                          torch.full((n, kp), S.SENTINEL, device=dev), torch.full((kp, npad), S.SENTINEL, device=dev))
    row = [W.data_ptr(), n, k, ws.data_ptr(), ws.stride(0), wts.data_ptr(), wts.stride(0), split_src, gap, b.data_ptr(),
           bs.data_ptr(), (k + 31) // 32, gW.data_ptr(), mW.data_ptr(), vW.data_ptr(), gb.data_ptr(), mb.data_ptr(), vb.data_ptr(),
           struct.unpack('<i', struct.pack('<f', 0.0))[0], -1, -1, int(wide), 0, 0]
    desc = torch.tensor([row], dtype=torch.int64, device=dev)
    desc2 = torch.tensor([[Ws3.data_ptr(), Ws3.stride(0), Wts3.data_ptr(), Wts3.stride(0), 11, 0, 0, 0]], dtype=torch.int64, device=dev)
    opt = torch.tensor([1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.001, 0.0], dtype=torch.float64, device=dev)
    acc = torch.zeros(L.ACC_COUNT, dtype=torch.float64, device=dev)
    W0 = W.clone()
    be.apply_multi_split(desc, None, torch.float16, opt, acc, desc2, None)
    be.refresh_shadow(W, R3, Rt3, split_src, split_src + gap, x3_exp=11)
    ref16 = torch.zeros_like(ws)
    torch.cuda.synchronize()
    cols = [c if c < split_src else c + gap for c in range(k)]
    ref16[:, cols] = W.half()
    return W0, W, ws, ref16, (Ws3, Wts3), (R3, Rt3)


@pytest.mark.parametrize('n,k,split_src,gap,wide', [(40, 72, 72, 0, 1), (40, 72, 72, 0, 0),      # ragged n and k, both paths of the kernel
                                                    (48, 72, 40, 8, 1), (40, 70, 30, 2, 0),      # a concat split: 16-byte / scalar path
                                                    (64, 256, 256, 0, 1)])                       # more than one tile along k and n
def test_apply_multi_writes_the_half_split_shadows(n, k, split_src, gap, wide):
    """The second shadow pair out of the optimizer launch is byte-equal to ase_hip_refresh_shadow(x3_exp = 11) of the updated
    masters (same split function), Ws and its transpose, padding untouched; the 16-bit shadow is still the rounded new weight.
    Both launches walk their tiles through csrc/shadow.h, so both pairs are also held to the torch packer of
    tests/ref_split_pack.py (sentinel-filled buffers: pad and gap positions included)."""
    W0, W, ws, ref16, got, ref = _apply_case(n, k, split_src, gap, wide)
    assert float((W - W0).abs().min()) > 0                                     # every weight moved (Adam's first step)
    assert torch.equal(ws.view(torch.int16), ref16.view(torch.int16))
    want = S.expected_pair(W.cpu(), 11, split_src, split_src + gap, tuple(got[0].shape), tuple(got[1].shape))
    for a, r, w in zip(got, ref, want):
        assert float(r.abs().max()) > 0
        assert torch.equal(a.view(torch.int32), r.view(torch.int32))
        assert torch.equal(a.view(torch.int32).cpu(), w) and torch.equal(r.view(torch.int32).cpu(), w)


def test_normalize_multi_f32_twin(be):
    """The f32 twin of rms_normalize_multi (the value path's input out of the branch's normalise launch) = rms_normalize into f32
    on the same rows, bit for bit: D = 12, a gathered index, the time-major remap; streams without a twin are not touched."""
    D, H, Nenv, M = 12, 5, 7, 23
    g = torch.Generator().manual_seed(6)
    srcs = [(torch.randn(H * Nenv, 16, generator=g) * 3).cuda() for _ in range(3)]
    idx = torch.randperm(H * Nenv, generator=g)[:M].to(torch.int32).cuda()
    streams = [(srcs[0], None, (0, 0)), (srcs[1], idx, (0, 0)), (srcs[2], idx, (H, Nenv))]
    means = [(torch.randn(D, generator=g) * 0.3).cuda() for _ in range(3)]
    stds = [(torch.rand(D, generator=g) * 0.5 + 0.05).cuda() for _ in range(3)]          # (small: some values reach the clamp)
    outs = [torch.zeros(M, 16, dtype=torch.float16, device='cuda') for _ in range(3)]
    ref16 = [torch.zeros(M, 16, dtype=torch.float16, device='cuda') for _ in range(3)]
    twin, ref32 = torch.full((M + 1, 16), 7.0, device='cuda'), torch.full((M + 1, 16), 7.0, device='cuda')
    be.rms_normalize_multi(streams, D, M, means, stds, ref16)
    be.rms_normalize(srcs[2], D, idx, (H, Nenv), M, means[2], stds[2], [ref32])
    be.rms_normalize_multi_twin(streams, D, M, means, stds, outs, [None, None, twin])
    torch.cuda.synchronize()
    assert float((ref32[:M, :D].abs() == 5).float().mean()) > 0 and float(ref32[:M, :D].abs().min()) < 1
    assert torch.equal(twin.view(torch.int32), ref32.view(torch.int32))          # (pad columns and the row past M: untouched)
    for a, b in zip(outs, ref16):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(outs[2][:, :D], ref32[:M, :D].half())


@pytest.mark.parametrize('gp_stream,capture', [(True, None), (False, None), (False, 'hipgraph')])
def test_engine_gp_fuse_on_against_off(gp_stream, capture, golden_dir):
    """The tiny fixture in f16 storage with gp_f32 = 'x3', multi-stream, two steps (the second on the weights the fused optimizer
    launch wrote, half-split shadows included): gp_fuse on computes what off computes - the exact masks, the seed and the 16-bit
    chain bit for bit; losses and gradients within 1e-5 of the tensor's largest magnitude, because two runs on a GPU add their
    f32 / f64 atomics in another order.  The weight bound (5 % of a learning-rate step, the golden checks' bound) says little by
    itself: Adam's first steps move every weight by about one learning rate whatever the gradient's size - the gradients carry
    the comparison, the weights only show that the same optimizer step ran.  capture = 'hipgraph': only the SCHEDULE a captured
    graph needs (serial prologue, no cross-step head, no own stream for the value path) in both settings - nothing is captured
    here.  Real captures are tests/test_gpu_agent.py's, which run the default (gp_fuse on); with gp_fuse off the launch sequence
    is the one those tests captured before this option existed, launch for launch."""
    from ase_amd.backend import HipBackend
    G = torch.load(os.path.join(golden_dir, 'ase_tiny.pt'), weights_only=False)
    out = {}
    for fuse in (False, True):
        _, eng, out[fuse] = run_steps(G, HipBackend(), steps=2, device='cuda', sync=torch.cuda.synchronize,
                                      engine_opts={'gp_fuse': fuse, 'gp_stream': gp_stream},
                                      cfg_extra={'graph_capture': capture} if capture else None)
        assert eng.multi_stream and eng._gp_fuse == fuse and eng._gp_split == fuse and eng._gp_side == gp_stream
        assert eng._xstep == (capture is None)
    assert float(out[True][0]['res']['disc_grad_penalty']) > 0
    lr = float(G['cfg']['learning_rate'])
    assert_same_step(out[True][0], out[False][0], 'step 0', exact=False, lr=lr)
    assert_same_step(out[True][1], out[False][1], 'step 1', exact=False, lr=lr)
