"""Exact reference of ase_hip_gemm_nt and the builder of its exact-operand cases - TEST INFRASTRUCTURE ONLY (CPU, torch).

The NT kernels accumulate in f32.  With INTEGER operands whose sums of |a| |b| stay below 2^24 every partial sum is an integer
f32 holds exactly, in any order; with a power-of-two alpha and a bias in multiples of 0.5 the pre-conversion value is exact too.
What a launch stores is then ONE correctly rounded conversion of a known number, so a kernel can be compared with torch.equal -
per element, per mask bit and per column sum - instead of under a tolerance.

Two parts:
  nt_reference(...)   the contract of include/ase_hip.h ("Dense layers") evaluated in f64: C, the mask_out words, the column sums.
                      It is written from the header, not from tests/emu_backend.py; tests/test_gemm_ref.py holds the two together.
  cases() / build()   the list of leaf shapes x storage modes x epilogue variants, and for a case its seeded operands + expected
                      outputs.  build() ASSERTS the conditions that make the comparison bitwise (and that make it bite: negative
                      values, stored zeros, bf16 outputs the conversion changes, exact round-to-nearest-even ties).  A case that
                      misses a condition gets other operand ranges (Case.spread), never a weaker condition.
"""
import math
from collections import OrderedDict
from dataclasses import dataclass, replace

import torch

from ase_amd.lib import (ACT_NONE, ACT_RELU, AUX_NONE, AUX_RELU_BITS, AUX_RELU_MASK, AUX_TANH_GRAD, BF16, F16, F32, F32H3,
                         F32X3)

EXACT = float(2 ** 24)            # integers below it are exact in f32
F16_MAX = 65504.0
STORE_DTYPE = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32, 'x3': torch.float32, 'h3': torch.float32}
STORE_CODE = {'bf16': BF16, 'f16': F16, 'f32': F32, 'x3': F32X3, 'h3': F32H3}
BITS_SENTINEL = 0x5A5A5A5A        # aux words / rows no valid output row maps to


# ------------------------------------------------------------------------------------------------------------------ reference
def pack_bits(keep):
    """bool [R, 32 W] -> int32 words [R, W]: bit n % 32 of word [m, n / 32] = keep[m, n]."""
    R, C = keep.shape
    assert C % 32 == 0
    # (disjoint bits, the top one worth -2^31 in int32: the sum never leaves the type)
    weights = torch.tensor([1 << i for i in range(31)] + [-(1 << 31)], dtype=torch.int32)
    return (keep.reshape(R, C // 32, 32).to(torch.int32) * weights).sum(-1, dtype=torch.int32)


def unpack_bits(words, N):
    """int32 words [R, W] -> bool [R, N]."""
    sh = torch.arange(32, dtype=torch.int32)
    return ((words.unsqueeze(-1) >> sh) & 1).reshape(words.shape[0], -1)[:, :N].bool()


def _aux_rows(aux, row0, rows, aux_split, aux_delta):
    """Rows of the mask operand as the output rows row0 .. row0 + rows read them: m >= aux_split (> 0) reads row m - aux_delta."""
    if aux_split > 0:
        m = torch.arange(row0, row0 + rows)
        return aux[torch.where(m >= aux_split, m - aux_delta, m)]
    return aux[row0:row0 + rows]


def nt_value(P, M, N, bias=None, alpha=1.0, factor=1.0, act=ACT_NONE, aux=None, aux_mode=AUX_NONE, aux_split=0, aux_delta=0,
             row0=0):
    """(the f64 value a launch converts and stores, the pre-activation z): z = alpha * factor * P + bias -> ReLU -> mask operand.
    P = the rows row0 .. row0 + M of A @ B.T as f64 [M, N] (aux is always the whole operand)."""
    assert P.dtype == torch.float64 and P.shape == (M, N)
    z = P * (float(alpha) * float(factor))
    if bias is not None:
        z = z + bias[:N].double()
    if act == ACT_RELU:
        v = z.clamp_min(0.0)
    else:
        assert act == ACT_NONE, "only the exact activations have an exact reference"
        v = z
    if aux_mode == AUX_RELU_MASK:
        v = v * (_aux_rows(aux, row0, M, aux_split, aux_delta)[:, :N] > 0)
    elif aux_mode == AUX_RELU_BITS:
        v = v * unpack_bits(_aux_rows(aux, row0, M, aux_split, aux_delta), N)
    elif aux_mode == AUX_TANH_GRAD:
        a = _aux_rows(aux, row0, M, aux_split, aux_delta)[:, :N].double()
        v = v * (1.0 - a * a)
    else:
        assert aux_mode == AUX_NONE
    return v, z


def nt_store(v, out_dtype, colsum_n=0, want_mask=False):
    """ONE conversion of the value to out_dtype (round to nearest even; half saturates at +-65504; v must be exact in f32, which
    build() asserts, so that the step through f32 rounds nothing), then mask_out bit = stored > 0 and colsum = f64 sums of the
    stored values.  Returns (C, mask words int32 [M, N / 32] or None, column sums f64 [colsum_n] or None)."""
    v = v.to(torch.float32)
    C = v.clamp(-F16_MAX, F16_MAX).to(torch.float16) if out_dtype == torch.float16 else v.to(out_dtype)
    mask = pack_bits(C > 0) if want_mask else None
    cs = C[:, :colsum_n].double().sum(0) if colsum_n > 0 else None
    return C, mask, cs


def nt_reference(P, M, N, out_dtype, colsum_n=0, want_mask=False, **kw):
    """The contract of ase_hip_gemm_nt in f64: (C, mask_out words, column sums) - nt_value, then nt_store."""
    return nt_store(nt_value(P, M, N, **kw)[0], out_dtype, colsum_n, want_mask)


# ---------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    leaf: str                 # the kernel leaf the SHAPE was chosen for
    kid: int                  # ase_hip_gemm_nt_kernel_id of the shape in this storage mode
    M: int
    N: int
    K: int
    store: str                # 'bf16' | 'f16' | 'f32' | 'x3' (ASE_F32X3) | 'h3' (ASE_F32H3)
    variant: str
    act: int = ACT_NONE
    aux_mode: int = AUX_NONE
    bias: bool = True
    alpha: float = 1.0
    factor: float = 0.0       # != 0: a scale record {factor, 0} rides as alpha_dev
    colsum_n: int = 0
    mask_out: bool = False
    out_f32: bool = False
    stacked: bool = False
    saturate: bool = False    # f16: one element of the last valid row and column is driven past 65504
    spread: float = 300.0     # target standard deviation of A.B^T (bf16 keeps integers up to 256: a third of the outputs round)
    exps: tuple = None        # 'h3': (ea, eb)

    @property
    def id(self):
        return f'{self.leaf}-{self.M}x{self.N}x{self.K}-{self.store}-{self.variant}'

    @property
    def out_dtype(self):
        return torch.float32 if self.out_f32 else STORE_DTYPE[self.store]


# (id, leaf, shapes): the smallest shapes that reach each leaf; ids are asserted against the library by the tests
LEAVES_16 = [
    (0, 'n64', [(1, 4, 32), (70, 36, 32)]),
    (1, 't128-64B', [(130, 132, 32), (130, 128, 96)]),
    (1, 't128-128B', [(16300, 512, 64), (16300, 516, 64)]),
    (4, 't64x128', [(8200, 448, 64), (8200, 452, 64)]),
    (5, 't64', [(130, 128, 64), (130, 96, 64), (130, 132, 64)]),
    (2, 'phased256', [(32700, 512, 64), (32700, 512, 128), (32700, 512, 192)]),
    (2, 'phased256-m65500', [(65500, 256, 64)]),
    (2, 'wave4', [(65536, 256, 64)]),        # the 4-wave kernel takes M >= 65536 only: 65500 rows stay on the 8-wave kernel
    (2, 'wave4-ragged', [(65600, 1024, 64)]),        # ... and the smallest grid with a ragged last tile that still reaches it
    (6, 'phased192', [(49000, 256, 64), (49000, 256, 192)]),
]
LONG_K_16 = [(2, 'phased256-longk', (32700, 512, 1408)), (6, 'phased192-longk', (49000, 256, 1408))]
LEAVES_32 = [
    (0, 'n64', [(1, 4, 16), (70, 36, 16)]),
    (1, 't128-64B', [(130, 132, 48)]),
    (1, 't128-128B', [(16300, 516, 32)]),
    (4, 't64x128', [(8200, 452, 32)]),
    (5, 't64', [(130, 132, 32)]),
    (3, 'lockstep256-128B', [(49000, 256, 32)]),
    (3, 'lockstep256-64B', [(49000, 256, 48)]),
]

# variant -> fields.  On a shape whose N is a whole number of wave tiles the launches rows_epi() admits (16-bit output, no column
# sums, act <= ReLU, mask operand absent or a bit matrix, mask_out only behind ReLU) take the row-per-lane epilogue, every other
# variant the LDS-slab epilogue; on every other shape all of them take the slab.
VARIANTS = OrderedDict([
    ('plain_bias', dict()),
    ('plain_nobias_a4', dict(bias=False, alpha=4.0)),
    ('relu_a05', dict(act=ACT_RELU, alpha=0.5)),
    ('maskout_relu', dict(act=ACT_RELU, mask_out=True)),
    ('maskout_none', dict(mask_out=True, alpha=4.0)),
    # (column sums over up to 65536 rows must stay below 2^24 units: alpha = unit = 0.5 behind ReLU, or no bias and a narrower spread)
    ('maskout_relu_colsum', dict(act=ACT_RELU, mask_out=True, colsum_n=-1, alpha=0.5)),
    ('maskout_none_colsum', dict(mask_out=True, colsum_n=-6, bias=False, spread=200.0)),
    ('colsum_n', dict(act=ACT_RELU, colsum_n=-1, alpha=0.5)),
    ('colsum_n5', dict(colsum_n=-6, bias=False, spread=200.0)),
    ('aux_relu_mask', dict(aux_mode=AUX_RELU_MASK)),
    ('aux_tanh_grad', dict(aux_mode=AUX_TANH_GRAD, bias=False)),
    ('aux_bits', dict(aux_mode=AUX_RELU_BITS)),
    ('aux_bits_stacked', dict(aux_mode=AUX_RELU_BITS, stacked=True, bias=False, alpha=4.0)),
    ('out_f32', dict(act=ACT_RELU, alpha=0.5, out_f32=True)),
    ('scale_record', dict(alpha=4.0, factor=0.5)),
    ('saturate', dict(saturate=True)),
    ('saturate_slab', dict(saturate=True, aux_mode=AUX_RELU_MASK)),
])
WAVE4_RAGGED = ('maskout_relu', 'aux_bits')      # 67 M outputs per launch: the two row-per-lane variants that use every piece of it
LONG_K = ('plain_bias', 'aux_relu_mask')          # rows / slab; alpha = 0.5


def _variants(M, N, store, names=None):
    for name, f in VARIANTS.items():
        if names is not None and name not in names:
            continue
        if f.get('mask_out') and N % 32 != 0:
            continue
        if f.get('out_f32') and store not in ('bf16', 'f16'):
            continue
        if f.get('saturate') and store != 'f16':
            continue
        if f.get('stacked') and M < 8:
            continue                                  # (a stacked block needs rows on both sides of aux_split)
        f = dict(f)
        if f.get('colsum_n', 0) < 0:
            f['colsum_n'] = N + 1 + f['colsum_n']     # -1: N, -6: N - 5
            if f['colsum_n'] <= 0:
                continue
        yield name, f


def cases():
    out = []
    for kid, leaf, shapes in LEAVES_16:
        for (M, N, K) in shapes:
            only = WAVE4_RAGGED if leaf == 'wave4-ragged' else None
            for name, f in _variants(M, N, 'bf16', only):
                for store in ('bf16', 'f16'):
                    out.append(Case(leaf, kid, M, N, K, store, name, **f))
            for name, f in _variants(M, N, 'f16', only):
                if f.get('saturate'):
                    out.append(Case(leaf, kid, M, N, K, 'f16', name, **f))
    for kid, leaf, (M, N, K) in LONG_K_16:
        for name, f in _variants(M, N, 'bf16', LONG_K):
            for store in ('bf16', 'f16'):
                out.append(Case(leaf, kid, M, N, K, store, name, **dict(f, alpha=0.5, spread=1000.0)))
    for kid, leaf, shapes in LEAVES_32:
        for (M, N, K) in shapes:
            for name, f in _variants(M, N, 'f32'):
                for store in ('f32', 'x3', 'h3'):
                    out.append(Case(leaf, kid, M, N, K, store, name, exps=None if store != 'h3' else (), **f))
                if name == 'plain_bias':             # the half split once more with unscaled operands
                    out.append(Case(leaf, kid, M, N, K, 'h3', 'plain_bias_e00', exps=(0, 0), **f))
    return out


def leaf_shapes():
    """[(M, N, K, dtype code, kernel id)] of every leaf shape, for the check against ase_hip_gemm_nt_kernel_id."""
    out = []
    for kid, _, shapes in LEAVES_16:
        out += [(M, N, K, code, kid) for (M, N, K) in shapes for code in (BF16, F16)]
    out += [(M, N, K, code, kid) for kid, _, (M, N, K) in LONG_K_16 for code in (BF16, F16)]
    for kid, _, shapes in LEAVES_32:
        out += [(M, N, K, code, kid) for (M, N, K) in shapes for code in (F32, F32X3, F32H3)]
    return out


# -------------------------------------------------------------------------------------------------------------------- builder
class _LRU(OrderedDict):
    def __init__(self, n):
        super().__init__()
        self.n = n

    def fetch(self, key, make):
        if key in self:
            self.move_to_end(key)
            return self[key]
        v = self[key] = make()
        while len(self) > self.n:
            self.popitem(last=False)
        return v


_OPERANDS, _AUX, _VALUE = _LRU(3), _LRU(3), _LRU(2)


def _unit(c):
    """The smallest power of two present in the pre-conversion value."""
    a = c.alpha * (c.factor or 1.0)
    u = min(a, 0.5) if c.bias else a
    return u * 0.25 if c.aux_mode == AUX_TANH_GRAD else u


def operand_range(c):
    """A, B are uniform integers in [-n, n] (variance n (n + 1) / 3 each): n from the target spread,
    sigma(alpha' A.B^T) / alpha' = sqrt(K) * n (n + 1) / 3."""
    t = c.spread / math.sqrt(c.K)
    return max(1, round((-1.0 + math.sqrt(1.0 + 12.0 * t)) / 2.0))


def _make_operands(M, N, K, n, seed, saturate):
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-n, n + 1, (M, K), generator=g).double()
    B = torch.randint(-n, n + 1, (N, K), generator=g).double()
    bias = torch.randint(-8, 9, (N,), generator=g).double() * 0.5
    bias[torch.rand(N, generator=g) < 0.5] = 0.0
    if M >= 8:                                       # stored exact zeros: all-zero rows of A over zero bias entries
        A[torch.randperm(M, generator=g)[:max(1, M // 25)]] = 0.0
    else:
        B[0] = 0.0
        bias[0] = 0.0
    if saturate:                                     # one product past half's range, in the last valid row and column
        A[M - 1, 0] = 512.0
        B[N - 1, 0] = 256.0
        bias[N - 1] = 0.5
    P = torch.cat([A[i:i + 8192] @ B.t() for i in range(0, M, 8192)])
    # an upper bound of max_mn sum_k |a| |b| (Hoelder, the tighter of the two sides)
    bound = float(min(A.abs().sum(1).max() * B.abs().max(), A.abs().max() * B.abs().sum(1).max()))
    return A.float(), B.float(), bias.float(), P, bound


def _make_aux(M, N, mode, seed, saturate):
    g = torch.Generator().manual_seed(seed + 77)
    if mode == AUX_RELU_MASK:
        a = torch.randint(-1, 3, (M, N), generator=g).float()
    elif mode == AUX_TANH_GRAD:
        a = torch.randint(-2, 3, (M, N), generator=g).float() * 0.5
    else:
        return pack_bits(torch.randint(0, 2, (M, (N + 31) // 32 * 32), generator=g).bool())
    if saturate:
        a[M - 1, N - 1] = 1.0
    return a


def stacked_rows(M):
    """(aux_split, aux_delta) of the stacked variant: the last quarter of the rows re-reads earlier rows, neither a tile multiple."""
    return M - M // 4, M // 4 + M // 8


class Built:
    pass


def _build(c, attempt):
    assert not (c.saturate and c.store != 'f16')
    n = operand_range(c)
    seed = c.M * 7 + c.N * 3 + c.K + 100003 * attempt
    A, B, bias, P, bound = _OPERANDS.fetch((c.M, c.N, c.K, n, seed, c.saturate),
                                           lambda: _make_operands(c.M, c.N, c.K, n, seed, c.saturate))
    b = Built()
    b.case, b.A, b.B, b.bias = c, A, B, (bias if c.bias else None)
    b.aux, b.aux_split, b.aux_delta = None, 0, 0
    if c.aux_mode != AUX_NONE:
        aux = _AUX.fetch((c.M, c.N, c.aux_mode, seed, c.saturate), lambda: _make_aux(c.M, c.N, c.aux_mode, seed, c.saturate))
        if c.stacked:
            b.aux_split, b.aux_delta = stacked_rows(c.M)
            assert 0 < b.aux_delta <= b.aux_split < c.M
            aux = aux.clone()
            aux[b.aux_split:] = BITS_SENTINEL if c.aux_mode == AUX_RELU_BITS else 3.0      # rows no valid m maps to
        b.aux = aux
    factor = c.factor or 1.0
    a = c.alpha * factor
    unit = _unit(c)

    def value():                                     # (in row blocks that stay in the cache: the same f64 arithmetic, a third of the time)
        v32, neg = torch.empty(c.M, c.N), 0
        for r in range(0, c.M, 2048):
            m = min(2048, c.M - r)
            v, z = nt_value(P[r:r + m], m, c.N, bias=b.bias, alpha=c.alpha, factor=factor, act=c.act, aux=b.aux,
                            aux_mode=c.aux_mode, aux_split=b.aux_split, aux_delta=b.aux_delta, row0=r)
            v32[r:r + m] = v
            assert bool((v32[r:r + m].double() == v).all()), 'the value before the conversion is not exact in f32'
            neg += int((z < 0).sum())
        return v32, neg / (c.M * c.N)
    # (the twin cases of a variant - bf16 / f16, f32 / x3 / h3 - share the value; v32 IS the f64 value from here on)
    v32, negative = _VALUE.fetch((replace(c, store='', leaf='', exps=None), attempt), value)
    b.C, b.mask, b.colsum = nt_store(v32, c.out_dtype, c.colsum_n, c.mask_out)

    # ---- the conditions that make the comparison bitwise
    assert math.log2(c.alpha).is_integer() and math.log2(factor).is_integer()
    assert bound < EXACT, ('sum |a| |b|', bound)
    assert (a * bound + (float(bias.abs().max()) if c.bias else 0.0)) / unit < EXACT
    if c.colsum_n > 0:
        assert float(b.C[:, :c.colsum_n].double().abs().sum(0).max()) / unit < EXACT, 'column sums of |stored| reach 2^24 units'
        assert bool((b.colsum.float().double() == b.colsum).all())
    if c.store == 'h3':
        assert c.exps and n * 2.0 ** c.exps[0] < F16_MAX and n * 2.0 ** c.exps[1] < F16_MAX
    # ---- and the ones that make it bite
    assert negative >= 0.10, 'fewer than 10 % negative values before ReLU'
    assert float((b.C == 0).float().mean()) >= 0.01, 'fewer than 1 % stored exact zeros'
    big = float(v32.abs().max())
    if c.saturate:
        assert float(v32[c.M - 1, c.N - 1]) > F16_MAX and float(b.C[c.M - 1, c.N - 1]) == F16_MAX
        assert int((v32.abs() >= F16_MAX).sum()) == 1
    else:
        assert big < F16_MAX
    if c.out_dtype != torch.float32:
        ch = b.C.float() != v32
        if c.saturate:
            ch[c.M - 1, c.N - 1] = False
        # a tie: the exact value sits half way between two neighbours of the storage type - its distance to the stored value is
        # half the spacing at the value, 2^(floor(log2 |v|) - p), p = 8 / 11 significand bits (looked for among the changed ones)
        p = 8 if c.store == 'bf16' else 11
        vc, sc = v32[ch].double(), b.C[ch].double()
        tie = (sc - vc).abs() == torch.exp2(torch.floor(torch.log2(vc.abs())) - p)
        b.rounded, b.ties = vc.numel() / v32.numel(), int(tie.sum())
        if c.store == 'bf16':
            assert b.rounded >= 0.05, ('bf16: fewer than 5 % of the outputs are changed by the conversion', b.rounded)
            assert b.ties >= 1, 'bf16: no exact round-to-nearest-even tie'
        elif c.alpha >= 32 or c.K == 1408:
            assert b.ties >= 1, 'f16: no exact tie'
    return b


def h3_exps(c):
    """(ea, eb) of an ASE_F32H3 case: the largest exponents <= (12, 11) that keep |a| 2^ea, |b| 2^eb inside half's range."""
    n = operand_range(c)
    e = int(math.floor(math.log2(65503.0 / n)))
    return min(12, e), min(11, e)


def build(c):
    """Operands + expected outputs of a case.  Tiny cases (a handful of outputs) try further seeds until the conditions hold -
    the draw is still a function of the case alone; everything else must hold on its first draw."""
    if c.store == 'h3' and not c.exps:
        c = replace(c, exps=h3_exps(c))
    tries = 64 if c.M * c.N < 4096 else 1
    for attempt in range(tries):
        try:
            return _build(c, attempt)
        except AssertionError:
            if attempt == tries - 1:
                raise


# --------------------------------------------------------------------------------------------------------------------- runner
C_SENTINEL, CS_INIT = -7.0, 3.0
_DEVICE_OPERANDS = _LRU(2)


def _padded(x, dt, pad, dev):
    """x [R, K] as a view of a [R, K + pad] buffer whose padding holds a non-zero sentinel (leading dimension > K)."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), 7.0, dtype=dt)
    buf[:, :x.shape[1]] = x.to(dt)
    return buf.to(dev)[:, :x.shape[1]]


def launch_and_check(be, b, dev='cpu'):
    """One gemm_nt launch of a built case on backend `be` (HipBackend, or the emulator on the CPU) into views of larger,
    sentinel-filled buffers - ldc > N with a column offset, rows after M, ldmask > N / 32, colsum longer than colsum_n, lda > K -
    and the bitwise comparison with the expected outputs.  Returns the number of elements compared."""
    c = b.case
    M, N, K = c.M, c.N, c.K
    dt = STORE_DTYPE[c.store]
    pad = 16 // torch.empty(0, dtype=dt).element_size()
    kw = {}

    def operands():
        A = _padded(b.A, dt, pad, dev)
        if c.store == 'h3':
            B = torch.zeros(N, K, dtype=dt, device=dev)
            be.refresh_shadow(b.B.to(dev), B, None, K, K, x3_exp=c.exps[1])
        else:
            B = _padded(b.B, dt, 2 * pad, dev)
        return A, B, b.A, b.B                         # (the sources ride along: their ids are the key)
    A, B = _DEVICE_OPERANDS.fetch((id(b.A), id(b.B), c.store, c.exps, str(dev)), operands)[:2]
    if c.store == 'h3':
        kw['x3_exps'] = c.exps
    Cbuf = torch.full((M + 3, N + 24), C_SENTINEL, dtype=c.out_dtype, device=dev)
    Cm = Cbuf[:M, 8:8 + N]
    W = N // 32
    Wbuf = Wm = cbuf = rec = aux = None
    if c.mask_out:
        Wbuf = torch.full((M + 2, W + 3), BITS_SENTINEL, dtype=torch.int32, device=dev)
        Wm = Wbuf[:M, 1:1 + W]
    if c.colsum_n > 0:
        cbuf = torch.full((c.colsum_n + 13,), CS_INIT, dtype=torch.float32, device=dev)
    if c.factor or c.saturate:
        rec = torch.tensor([c.factor or 1.0, 0.0], dtype=torch.float32, device=dev)
    if c.aux_mode == AUX_RELU_BITS:
        abuf = torch.full((b.aux.shape[0], b.aux.shape[1] + 2), BITS_SENTINEL, dtype=torch.int32)
        abuf[:, 1:-1] = b.aux
        aux = abuf.to(dev)[:, 1:-1]
    elif c.aux_mode != AUX_NONE:
        aux = _padded(b.aux, dt, pad, dev)
    be.gemm_nt(A, B, Cm, M, N, K, bias=None if b.bias is None else b.bias.to(dev), aux=aux, aux_mode=c.aux_mode,
               colsum=None if cbuf is None else cbuf[4:], colsum_n=c.colsum_n, act=c.act, alpha=c.alpha,
               aux_split=b.aux_split, aux_delta=b.aux_delta, mask_out=Wm, alpha_dev=rec, **kw)

    got = Cbuf.cpu()
    if not torch.equal(got[:M, 8:8 + N], b.C):
        bad = (got[:M, 8:8 + N] != b.C).nonzero()
        raise AssertionError((c.id, 'C: elements not bitwise equal', len(bad), 'of', M * N, 'first (m, n)', bad[0].tolist(),
                              'got', float(got[bad[0, 0], 8 + bad[0, 1]]), 'want', float(b.C[bad[0, 0], bad[0, 1]])))
    for name, edge in (('rows after M', got[M:]), ('columns before', got[:M, :8]), ('columns after N', got[:M, 8 + N:])):
        assert bool((edge == C_SENTINEL).all()), (c.id, 'C: written outside [M, N]', name)
    n = M * N
    if c.mask_out:
        w = Wbuf.cpu()
        if not torch.equal(w[:M, 1:1 + W], b.mask):
            bad = (unpack_bits(w[:M, 1:1 + W], N) != unpack_bits(b.mask, N)).nonzero()
            raise AssertionError((c.id, 'mask_out: wrong bits', len(bad), 'of', M * N, 'first (m, n)', bad[0].tolist()))
        for name, edge in (('rows after M', w[M:]), ('word before', w[:M, :1]), ('words after', w[:M, 1 + W:])):
            assert bool((edge == BITS_SENTINEL).all()), (c.id, 'mask_out: written outside [M, N / 32]', name)
        n += M * N
    if c.colsum_n > 0:
        s = cbuf.cpu()
        want = torch.full_like(s, CS_INIT)
        want[4:4 + c.colsum_n] += b.colsum.float()
        assert torch.equal(s, want), (c.id, 'colsum', int((s != want).sum()), 'of', c.colsum_n)
        n += c.colsum_n
    if rec is not None:
        r = rec.cpu()
        assert float(r[0]) == (c.factor or 1.0), (c.id, 'the record\'s factor was written')
        if c.saturate:
            assert float(r[1]) > 0.0, (c.id, 'a stored 65504 was not reported')
        else:
            assert float(r[1]) == 0.0, (c.id, 'overflow reported', float(r[1]))
    return n
