"""ase_hip_gemm_nt_stacked: two row blocks of one A / C pair with an epilogue each - the forward's duties on rows [0, split), the
penalty chain's on rows [split, M) - against the two plain ase_hip_gemm_nt launches it replaces and against the exact reference of
tests/ref_gemm.py.  Operands are small integers, alpha and the record factors powers of two, the bias in multiples of 0.5: every
partial sum is exact in f32 in ANY order, so the native path (one launch of the phased 256 x 256 kernel), the fallback (two launches
inside the library) and the two launches of the test itself must agree bit for bit although they run different tile kernels."""
import ctypes
import functools

import pytest
import torch

from ase_amd import lib as L
from tests import ref_gemm as R

pytestmark = pytest.mark.gpu

DT = {'f16': torch.float16, 'bf16': torch.bfloat16}
ALPHA, F1, ALPHA2, F2 = 1.0, 0.5, 4.0, 0.5        # alpha * its record's factor: 0.5 for the first block, 2 for the second
C_SENT = -7.0
# native: kernel 2 of the whole shape and split in whole 256-row tiles - one, two and five K-tiles (prologue, tail, steady loop)
NATIVE = [(16384, 1024, K, s) for K in (64, 128, 320) for s in (256, 12288, 16128)]
# fallback: split off the tile grid; generic tiles (5: 64 x 64, 4: 64 x 128, 1: 128 x 128); the narrow-output tile
FALLBACK = [(16384, 1024, 128, 12352), (512, 256, 128, 256), (4096, 1024, 128, 2048), (8192, 1024, 128, 4096), (256, 64, 64, 128)]


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend()


@functools.lru_cache(maxsize=2)
def _operands(M, N, K):
    """Integer operands in [-3, 3] (sum |a| |b| <= 9 K < 2^24), the bias, random mask words for EVERY row (a case uses the first
    M - split) and the exact product A.B^T in f64 - computed once per shape, on the device, by torch's f64 matmul."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    B = torch.randint(-3, 4, (N, K), generator=g).float()
    A[torch.randperm(M, generator=g)[:max(1, M // 25)]] = 0.0          # stored exact zeros
    bias = torch.randint(-8, 9, (N,), generator=g).float() * 0.5
    bias[bias == 0] = 0.5                                                # nonzero everywhere: a biased second block shows
    W = (N + 31) // 32
    aux = R.pack_bits(torch.randint(0, 2, (M, W * 32), generator=g).bool())
    P = (A.cuda().double() @ B.cuda().double().t()).cpu()
    assert 9 * K * 4.0 + 4.0 < R.F16_MAX
    return A, B, bias, aux, P


def _expected(M, N, K, split, dt):
    """ref_gemm's contract, block by block: (C, mask_out words of the first block)."""
    A, B, bias, aux, P = _operands(M, N, K)
    want_mask = N % 32 == 0
    c1, m1, _ = R.nt_reference(P[:split], split, N, dt, want_mask=want_mask, bias=bias, alpha=ALPHA, factor=F1, act=L.ACT_RELU)
    c2, _, _ = R.nt_reference(P[split:], M - split, N, dt, alpha=ALPHA2, factor=F2, aux=aux[:M - split], aux_mode=L.AUX_RELU_BITS)
    return torch.cat([c1, c2]), m1


def _buffers(M, N, dt):
    W = (N + 31) // 32
    C = torch.full((M + 2, N + 16), C_SENT, dtype=dt, device='cuda')
    words = torch.full((M + 2, W + 2), R.BITS_SENTINEL, dtype=torch.int32, device='cuda')
    return C, words


def _run(be, M, N, K, split, dt, stacked):
    """The stacked launch, or the two plain launches on the row ranges; returns (C buffer, mask word buffer, the two records)."""
    A, B, bias, aux, _ = _operands(M, N, K)
    Ad, Bd, bd = A.to('cuda', dt), B.to('cuda', dt), bias.cuda()
    auxd = aux[:M - split].cuda()
    Cb, Wb = _buffers(M, N, dt)
    Cm = Cb[:M, 8:8 + N]
    Wm = Wb[:M, 1:1 + (N + 31) // 32] if N % 32 == 0 else None
    r1 = torch.tensor([F1, 0.0], device='cuda')
    r2 = torch.tensor([F2, 0.0], device='cuda')
    if stacked:
        be.gemm_nt(Ad, Bd, Cm, M, N, K, bias=bd, act=L.ACT_RELU, mask_out=Wm, alpha=ALPHA, alpha_dev=r1,
                   stack=(split, auxd, ALPHA2, r2))
    else:
        be.gemm_nt(Ad[:split], Bd, Cm[:split], split, N, K, bias=bd, act=L.ACT_RELU, mask_out=None if Wm is None else Wm[:split],
                   alpha=ALPHA, alpha_dev=r1)
        be.gemm_nt(Ad[split:], Bd, Cm[split:], M - split, N, K, aux=auxd, aux_mode=L.AUX_RELU_BITS, alpha=ALPHA2, alpha_dev=r2)
    torch.cuda.synchronize()
    return Cb.cpu(), Wb.cpu(), r1.cpu(), r2.cpu()


def _check(be, M, N, K, split, store):
    dt = DT[store]
    W = (N + 31) // 32
    want_c, want_m = _expected(M, N, K, split, dt)
    got_c, got_w, r1, r2 = _run(be, M, N, K, split, dt, True)
    two_c, two_w, _, _ = _run(be, M, N, K, split, dt, False)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(got_c), bits(two_c)), 'C differs from the two plain launches'
    assert torch.equal(got_w, two_w), 'mask_out differs from the two plain launches'
    C = got_c[:M, 8:8 + N]
    # (by value, as tests/ref_gemm.py compares: the reference MULTIPLIES by the mask, a masked-out negative is its -0, the kernels' +0)
    assert torch.equal(C, want_c), ('C differs from the reference', int((C != want_c).sum()))
    # nothing outside [M, N]
    assert bool((got_c[M:] == C_SENT).all()) and bool((got_c[:, :8] == C_SENT).all()) and bool((got_c[:, 8 + N:] == C_SENT).all())
    # second-block rows carry no bias and no ReLU: they are the masked product alone - and some of it is negative
    A, B, bias, aux, P = _operands(M, N, K)
    keep = R.unpack_bits(aux[:M - split], N)
    assert torch.equal(C[split:].double(), (P[split:] * (ALPHA2 * F2) * keep).to(dt).double())
    assert bool((C[split:] < 0).any()) and bool((C[:split] >= 0).all()) and bool((C[:split] > 0).any())
    if N % 32 == 0:
        words = got_w[:M, 1:1 + W]
        assert torch.equal(words[:split], want_m), 'first-block bits'
        assert torch.equal(R.unpack_bits(words[:split], N), C[:split] > 0)
        assert bool((words[split:] == R.BITS_SENTINEL).all()), 'mask_out words of rows >= split were written'
        assert bool((got_w[M:] == R.BITS_SENTINEL).all()) and bool((got_w[:, 0] == R.BITS_SENTINEL).all()) and \
            bool((got_w[:, 1 + W:] == R.BITS_SENTINEL).all())
    # the records: factors untouched, nothing overflowed (each block was scaled by its own: the reference holds the two factors apart)
    assert r1.tolist() == [F1, 0.0] and r2.tolist() == [F2, 0.0]


@pytest.mark.parametrize('store', ['f16', 'bf16'])
@pytest.mark.parametrize('M,N,K,split', NATIVE)
def test_stacked_native(be, M, N, K, split, store):
    assert be.lib.ase_hip_gemm_nt_kernel_id(M, N, K, {'f16': L.F16, 'bf16': L.BF16}[store]) == 2 and split % 256 == 0
    _check(be, M, N, K, split, store)


@pytest.mark.parametrize('store', ['f16', 'bf16'])
@pytest.mark.parametrize('M,N,K,split', FALLBACK)
def test_stacked_fallback(be, M, N, K, split, store):
    _check(be, M, N, K, split, store)


@pytest.mark.parametrize('store', ['f16', 'bf16'])
def test_stacked_records_act_on_their_own_block(be, store):
    """Other factors in the two records: each block follows its own record alone."""
    M, N, K, split, dt = 16384, 1024, 64, 256, DT[store]
    A, B, bias, aux, P = _operands(M, N, K)
    Ad, Bd = A.to('cuda', dt), B.to('cuda', dt)
    out = {}
    for f1, f2 in ((1.0, 1.0), (2.0, 1.0), (1.0, 0.25)):
        C = torch.zeros(M, N, dtype=dt, device='cuda')
        r1, r2 = torch.tensor([f1, 0.0], device='cuda'), torch.tensor([f2, 0.0], device='cuda')
        be.gemm_nt(Ad, Bd, C, M, N, K, alpha=1.0, alpha_dev=r1, stack=(split, None, 1.0, r2))
        out[(f1, f2)] = C.double().cpu()
    base = out[(1.0, 1.0)]
    assert torch.equal(base, P.to(dt).double())
    assert torch.equal(out[(2.0, 1.0)][:split], (P[:split] * 2).to(dt).double()) and torch.equal(out[(2.0, 1.0)][split:], base[split:])
    assert torch.equal(out[(1.0, 0.25)][split:], (P[split:] * 0.25).to(dt).double()) and torch.equal(out[(1.0, 0.25)][:split], base[:split])


@pytest.mark.parametrize('store', ['f16', 'bf16'])
def test_stacked_non_finite(be, store):
    """Smallest native shape.  A NaN in a first-block row survives ReLU (torch.relu) and sets no mask_out bit; an inf in a second-block
    row makes that row's products inf / NaN, and the mask SELECTS: a zero bit stores 0.  Every other row is what it is without them."""
    M, N, K, split, dt = 16384, 1024, 64, 256, DT[store]
    A, B, bias, aux, _ = _operands(M, N, K)
    clean_c, clean_w, _, _ = _run(be, M, N, K, split, dt, True)
    A = A.clone()
    rn, ri = 3, split + 5
    A[rn, 0] = float('nan')
    A[ri, 0] = float('inf')
    Ad, Bd = A.to('cuda', dt), B.to('cuda', dt)
    C = torch.full((M, N), C_SENT, dtype=dt, device='cuda')
    words = torch.full((M, N // 32), R.BITS_SENTINEL, dtype=torch.int32, device='cuda')
    be.gemm_nt(Ad, Bd, C, M, N, K, bias=bias.cuda(), act=L.ACT_RELU, mask_out=words, alpha=0.5, stack=(split, aux[:M - split].cuda(), 2.0, None))
    torch.cuda.synchronize()
    C, words = C.cpu(), words.cpu()
    assert bool(torch.isnan(C[rn]).all()) and bool((words[rn] == 0).all())
    keep = R.unpack_bits(aux[ri - split:ri - split + 1], N)[0]
    assert bool((~keep).any()) and bool(keep.any())
    assert bool((C[ri][~keep] == 0).all()), 'a masked-out inf / NaN product was not stored as 0'
    kept = C[ri][keep].float()
    assert bool((~torch.isfinite(kept) | (kept.abs() >= 65504.0)).all())      # (f16 saturates an inf, keeps a NaN)
    rest = torch.ones(M, dtype=torch.bool)
    rest[[rn, ri]] = False
    assert torch.equal(C[rest].view(torch.int16), clean_c[:M, 8:8 + N][rest].view(torch.int16))
    assert torch.equal(words[:split][rest[:split]], clean_w[:M, 1:1 + N // 32][:split][rest[:split]])


def test_stacked_refusals(be):
    """ASE_EINVAL before any launch: split outside (0, M), a mask operand that is not the second block's, mask_out without ReLU,
    colsum, out_f32."""
    lib = be.lib
    M, N, K = 512, 256, 128
    A = torch.zeros(M, K, dtype=torch.float16, device='cuda')
    B = torch.zeros(N, K, dtype=torch.float16, device='cuda')
    C = torch.zeros(M, N, dtype=torch.float16, device='cuda')
    words = torch.zeros(M, N // 32, dtype=torch.int32, device='cuda')
    cs = torch.zeros(N, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(split=256, aux=None, aux_split=256, aux_delta=256, colsum=None, mask_out=None, act=L.ACT_NONE, aux_mode=L.AUX_NONE, out_f32=0):
        return lib.ase_hip_gemm_nt_stacked(p(A), K, p(B), K, p(C), N, None, None if aux is None else p(aux), N // 32, aux_split, aux_delta,
                                           None if colsum is None else p(colsum), N if colsum is not None else 0,
                                           None if mask_out is None else p(mask_out), N // 32, M, N, K, act, aux_mode, out_f32, 1.0, None,
                                           split, 1.0, None, L.F16, None)
    assert call() == 0
    assert call(aux=words, aux_mode=L.AUX_RELU_BITS) == 0
    assert call(mask_out=words, act=L.ACT_RELU) == 0
    for kw in (dict(split=0), dict(split=-256), dict(split=M), dict(split=M + 256),
               dict(aux=words, aux_mode=L.AUX_RELU_BITS, aux_split=0, aux_delta=0),          # the mask would cover the first block
               dict(aux=words, aux_mode=L.AUX_RELU_BITS, aux_split=128, aux_delta=128),
               dict(aux=C, aux_mode=L.AUX_RELU_MASK),
               dict(mask_out=words), dict(mask_out=words, act=L.ACT_TANH),
               dict(colsum=cs), dict(out_f32=1)):
        assert call(**kw) == -1 and b'gemm_nt_stacked' in lib.ase_hip_last_error(), kw
    torch.cuda.synchronize()
