"""The main loop of the ASE_F32H3 NT kernels (csrc/gemm_nt_kernels.h: the two-instruction A split, the pipelined K-tile, the scalar
DMA addressing), every output element compared bitwise.

  The split, made visible: B is the pre-split shadow of an identity matrix, so C[m, n] = f32(lo + hi) / sa of A[m, n] - the kernel's
      own split of tests/test_h3_split_rounding.py's edge list (and random values), against the numpy split.  A row that holds an
      element beyond half's range is NaN from end to end (inf times the identity's zeros), as the emulator has it.
  The pipeline's edges: exact-integer operands (tests/ref_gemm.py: bitwise in any order of accumulation) over 1 .. 5 K-tiles of
      both staged-row widths, row counts around the 64-row tile, the kernel ids 0, 4, 5 (and 1 for the 64-byte rows of a wide
      output), plain and with the fused epilogue duties.
      Kernel id 4 needs at least 512 tiles of 64 x 128 and fewer than 512 of 128 x 128: no N does that for M = 64, so its row
      counts are 65, 127 and 130, with N = 128 ceil(512 / ceil(M / 64))."""
import numpy as np
import pytest
import torch

from ase_amd import lib as L
from tests import ref_gemm as R
from tests.emu_backend import x3_half_product
from tests.test_gpu_gp_fuse import _bits, _convert
from tests.test_h3_split_rounding import edge_values, random_values, split_exact

pytestmark = pytest.mark.gpu

EB = 11


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(x3='f16')


# ------------------------------------------------------------------------------------------------------ the split, made visible
def _split_operand(M, K, ea):
    """A [M, K]: random values inside half's range after scaling; the finite edges on every other element of the rows m % 3 != 2
    (as many as fit, starting at edge number K so that the small shapes do not all take the same ones); one overflowing element
    in every row m % 3 == 2."""
    fin, ovf = edge_values(ea)
    A = (random_values(M * K, 1000 * M + K + ea) * np.float32(2.0 ** (9 - ea))).reshape(M, K)          # |sa x| in [2^-21, 2^15]
    rows = [m for m in range(M) if m % 3 != 2]
    flat = A[rows].reshape(-1)
    n = min(fin.size, (flat.size + 1) // 2)
    flat[0:2 * n:2] = np.roll(fin, -K)[:n]
    A[rows] = flat.reshape(len(rows), K)
    for i, m in enumerate(range(2, M, 3)):
        A[m, (7 * m) % K] = ovf[i % ovf.size]
    return A


@pytest.mark.parametrize('ea', (12, 6))
@pytest.mark.parametrize('K', (32, 64, 96, 160))
@pytest.mark.parametrize('M', (1, 63, 65, 130))
def test_split_made_visible(be, M, K, ea):
    A = _split_operand(M, K, ea)
    hi, lo = split_exact(A, ea)
    bad = ~(np.isfinite(hi) & np.isfinite(lo)).all(axis=1)
    assert bad.sum() == len(range(2, M, 3))
    # f32 accumulators start at +0: al bh, then ah bl = 0, then ah bh - one rounding of lo + hi (f64 holds the sum exactly)
    with np.errstate(invalid='ignore'):                      # (the overflowing rows: inf - inf)
        want = ((hi.astype(np.float64) + lo.astype(np.float64)).astype(np.float32) + np.float32(0.0)) * np.float32(2.0 ** -ea)
    want[bad] = np.nan
    emu = x3_half_product(torch.from_numpy(A), torch.eye(K), ea, EB).numpy()
    assert np.array_equal(np.isnan(emu), np.isnan(want))
    assert np.array_equal(emu[~bad].view(np.int32) & 0x7FFFFFFF, want[~bad].view(np.int32) & 0x7FFFFFFF)   # (f64 sums: no sign of zero)

    Bs = torch.zeros(K, K, device='cuda')
    be.refresh_shadow(torch.eye(K, device='cuda'), Bs, None, K, K, x3_exp=EB)
    C = torch.full((M + 1, K + 8), 7.0, device='cuda')
    be.gemm_nt(torch.from_numpy(A).cuda(), Bs, C[:M, :K], M, K, K, x3_exps=(ea, EB))
    got = C.cpu().numpy()
    assert np.all(got[M:] == 7.0) and np.all(got[:, K:] == 7.0)
    got = np.ascontiguousarray(got[:M, :K])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.int32)[ok], want.view(np.int32)[ok])
    assert int(ok.sum()) + int(np.isnan(want).sum()) == M * K


# ---------------------------------------------------------------------------------------------------------- the pipeline's edges
def _id4_n(M):
    return 128 * -(-512 // -(-M // 64))


K128, K64 = (32, 64, 96, 128, 160), (16, 32, 48, 64, 80)            # 1 .. 5 K-tiles of 128-byte / 64-byte staged rows
PLAIN = ([(0, M, 64, K) for M in (64, 65, 127, 130) for K in K64] +          # id 0 stages 64-byte rows whatever K is
         [(1, M, 132, K) for M in (64, 65, 127, 130) for K in (16, 48, 80)] +   # a wide output whose K is no whole 128-byte step
         [(5, M, 132, K) for M in (64, 65, 127, 130) for K in K128] +
         [(4, M, _id4_n(M), K) for M in (65, 127, 130) for K in K128])
EPILOGUES = [(kid, 130, N, 96, v) for kid, N in ((0, 64), (5, 160), (4, _id4_n(130))) for v in ('maskout_relu', 'aux_bits')]


def _case(kid, M, N, K, variant):
    return R.Case('h3loop', kid, M, N, K, 'h3', variant, exps=(), **R.VARIANTS[variant])


@pytest.mark.parametrize('kid,M,N,K,variant', [(*s, 'plain_bias') for s in PLAIN] + EPILOGUES,
                         ids=lambda v: str(v))
def test_k_tiles_and_row_counts(be, kid, M, N, K, variant):
    assert be.lib.ase_hip_gemm_nt_kernel_id(M, N, K, L.F32H3) == kid
    assert R.launch_and_check(be, R.build(_case(kid, M, N, K, variant)), dev=be.device) >= M * N


FUSED = [(0, 65, 64, 48), (0, 130, 64, 80), (5, 127, 160, 64), (5, 130, 160, 160), (4, 130, _id4_n(130), 32), (4, 65, _id4_n(65), 96)]


def _device(be, b):
    c = b.case
    Bs = torch.zeros(c.N, c.K, device='cuda')
    be.refresh_shadow(b.B.cuda(), Bs, None, c.K, c.K, x3_exp=c.exps[1])
    return b.A.cuda(), Bs


@pytest.mark.parametrize('kid,M,N,K', FUSED)
def test_fused_seed_launch(be, kid, M, N, K):
    """bias + ReLU + mask_out with the seed s w[n] [h > 0] in place of h and its f16 twin: the plain launch equals the exact
    reference, the fused launch the helpers' sequence on it."""
    assert be.lib.ase_hip_gemm_nt_kernel_id(M, N, K, L.F32H3) == kid
    b = R.build(_case(kid, M, N, K, 'maskout_relu'))
    A, Bs = _device(be, b)
    g = torch.Generator().manual_seed(M + K)
    width, s = N - 3, 0.0173
    w = torch.randn(width, generator=g).cuda()
    kw = dict(bias=b.bias.cuda(), act=L.ACT_RELU, x3_exps=b.case.exps)
    H, m0 = torch.zeros(M, N, device='cuda'), torch.zeros(M, N // 32, dtype=torch.int32, device='cuda')
    G0, T0 = torch.zeros(M, N, device='cuda'), torch.zeros(M, N, dtype=torch.float16, device='cuda')
    be.gemm_nt(A, Bs, H, M, N, K, mask_out=m0, **kw)
    be.gp_seed(H, w, G0, M, width, scale=s)
    _convert(be, G0, T0, M)
    G1, m1 = torch.full((M, N), 7.0, device='cuda'), torch.zeros(M, N // 32, dtype=torch.int32, device='cuda')
    T1 = torch.full((M, N), 7.0, dtype=torch.float16, device='cuda')
    be.gemm_nt(A, Bs, G1, M, N, K, mask_out=m1, seed=(w, s), twin=T1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(H.cpu(), b.C) and torch.equal(m0.cpu(), b.mask)
    assert torch.equal(m1, m0) and torch.equal(_bits(m1, N).bool(), H > 0)
    assert float(G0.abs().max()) > 0
    assert torch.equal(G1.view(torch.int32), G0.view(torch.int32))
    assert torch.equal(T1.view(torch.int16), T0.view(torch.int16))


@pytest.mark.parametrize('kid,M,N,K', FUSED)
def test_fused_chain_launch_with_twin(be, kid, M, N, K):
    """A consumed bit mask, the f32 output and its bf16 twin."""
    b = R.build(_case(kid, M, N, K, 'aux_bits'))
    A, Bs = _device(be, b)
    kw = dict(bias=b.bias.cuda(), aux=b.aux.cuda(), aux_mode=L.AUX_RELU_BITS, x3_exps=b.case.exps)
    C0, T0 = torch.zeros(M, N, device='cuda'), torch.zeros(M, N, dtype=torch.bfloat16, device='cuda')
    be.gemm_nt(A, Bs, C0, M, N, K, **kw)
    _convert(be, C0, T0, M)
    C1, T1 = torch.full((M, N), 7.0, device='cuda'), torch.full((M, N), 7.0, dtype=torch.bfloat16, device='cuda')
    be.gemm_nt(A, Bs, C1, M, N, K, twin=T1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(C0.cpu(), b.C)
    assert torch.equal(C1.view(torch.int32), C0.view(torch.int32))
    assert torch.equal(T1.view(torch.int16), T0.view(torch.int16))
    assert float((T0.float() != C0).float().mean()) > 0.01                   # the twin's conversion rounds


@pytest.mark.parametrize('kid,M,N,K', FUSED)
def test_fused_twin_only_and_sum_of_squares(be, kid, M, N, K):
    """No f32 store (the buffer stays untouched), an f16 twin, scale * factor * sum of the stored squares.  The stored values are
    integers times 4; a lane's f32 partial over 4 squares carries at most 4 * 2^-24 relative, everything behind it is f64: the
    fused launches, ase_hip_sqnorm and the f64 sum agree within 1e-6 relative (tests/test_gpu_gp_fuse.py's bound)."""
    b = R.build(_case(kid, M, N, K, 'plain_nobias_a4'))
    A, Bs = _device(be, b)
    scale = 3.0e-3
    dyn = torch.tensor([0.5, 0.0], device='cuda')
    kw = dict(alpha=b.case.alpha, x3_exps=b.case.exps)
    C0, T0 = torch.zeros(M, N, device='cuda'), torch.zeros(M, N, dtype=torch.float16, device='cuda')
    acc0 = torch.zeros(4, dtype=torch.float64, device='cuda')
    be.gemm_nt(A, Bs, C0, M, N, K, **kw)
    be.sqnorm(C0, M, N, acc0, 2, scale=scale, dyn=dyn)
    _convert(be, C0, T0, M)
    C1, T1 = torch.full((M, N), 7.0, device='cuda'), torch.full((M, N), 7.0, dtype=torch.float16, device='cuda')
    acc1 = torch.zeros(4, dtype=torch.float64, device='cuda')
    be.gemm_nt(A, Bs, C1, M, N, K, twin=T1, store=False, sq=(acc1, 2, scale, dyn), **kw)
    C2, acc2 = torch.full((M, N), 7.0, device='cuda'), torch.zeros(4, dtype=torch.float64, device='cuda')
    be.gemm_nt(A, Bs, C2, M, N, K, sq=(acc2, 2, scale, dyn), **kw)
    torch.cuda.synchronize()
    assert torch.equal(C0.cpu(), b.C)
    assert torch.equal(C1, torch.full_like(C1, 7.0))
    assert torch.equal(T1.view(torch.int16), T0.view(torch.int16))
    assert torch.equal(C2.view(torch.int32), C0.view(torch.int32))
    ref = scale * 0.5 * float((b.C.double() ** 2).sum())
    got0, got1, got2 = float(acc0[2]), float(acc1[2]), float(acc2[2])
    print('sum of squares: f64 %.12e  sqnorm %.12e  fused %.12e / %.12e' % (ref, got0, got1, got2))
    assert ref > 0 and float(dyn[1]) == 0
    for got in (got1, got2):
        assert abs(got - got0) <= 1e-6 * abs(got0) and abs(got - ref) <= 1e-6 * abs(ref), (got, got0, ref)
