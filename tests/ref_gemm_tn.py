"""Exact reference of ase_hip_gemm_tn / ase_hip_gemm_tn_grouped and the builder of their exact-operand cases - TEST INFRASTRUCTURE
ONLY (CPU, torch).  The weight-gradient twin of tests/ref_gemm.py.

The TN kernels split the contraction over M and let the partial sums meet in f32 atomics (or in the workspace fold) in an
unspecified order.  With INTEGER operands whose sums of |a| |b| stay below 2^24 every partial sum is an integer f32 holds exactly,
so the order cannot matter; with a power-of-two alpha and a G0 in multiples of alpha the stored value is exact too.  G and gbias
are therefore compared with torch.equal - also on the atomic paths, where a tolerance would have to leave the most slack.

  tn_reference(...)     the contract of include/ase_hip.h ("TN" GEMM, grouped launch) in f64, accumulated in row blocks.  Written
                        from the header, not from tests/emu_backend.py; tests/test_gemm_ref.py holds the two together.
  cases() / build()     single-problem shapes x storage modes x variants; build() ASSERTS what the bitwise comparison rests on and
                        what makes it bite.  A case that misses a condition gets other operand ranges, never a weaker condition.
  group_sets() ...      the grouped launches: sets of problems, some of which share their gradient buffers.

Buffers of a launch: A and B are views of larger buffers (lda > N, ldb > K) whose pitch columns and rows after M hold NaN; G is a
contiguous [n_real, k_real] window of a longer flat sentinel buffer and gbias a window of another - long enough that a row or a
column sum stored past n_real would land in the guard, not outside the allocation.  The pad columns the header names ([n_real, N)
of A, the concat gap and [k_real + gap, K) of B) hold zeros, or NaN in the `poison` variant: their content must never reach G.
"""
import ctypes
import math
import struct
from dataclasses import dataclass

import torch

from ase_amd.lib import BF16, F16, F32, F32X3
from tests.ref_gemm import EXACT, STORE_DTYPE, _LRU

STORE_CODE = {'bf16': BF16, 'f16': F16, 'f32': F32, 'x3': F32X3}
STORE_MAX = {'bf16': 256.0, 'f16': 2048.0}       # integers up to here are exact in the storage type
G_SENTINEL, B_SENTINEL = -7777.0, -5555.0
G_BEFORE, B_BEFORE = 3, 2
ROW_BLOCK = 8192
LARGE_M = 16384                                   # from here on the entries come from {-2 .. 2}


# ------------------------------------------------------------------------------------------------------------------ reference
def g_columns(k_real, split_src, split_dst):
    """Column of B that column j of G reads: the inverse of the header's kmap (k < split_src -> k; k >= split_dst -> k - gap)."""
    gap = split_dst - split_src
    return torch.tensor([j if j < split_src else j + gap for j in range(k_real)], dtype=torch.long)


def tn_sums(A, B, M, n_real, k_real, split_src, split_dst, bias_rows):
    """(sum_m A[m, n] B[m, k] as f64 [n_real, k_real] in G's layout, sum_{m < bias_rows} A[m, n] as f64 [n_real]), accumulated in
    row blocks so that no f64 copy of a whole operand exists.  Only the columns the contract names are read."""
    cols = g_columns(k_real, split_src, split_dst)
    assert int(cols.max()) < B.shape[1], 'k_real + gap exceeds K'
    br = bias_rows if bias_rows > 0 else M
    S = torch.zeros(n_real, k_real, dtype=torch.float64)
    sb = torch.zeros(n_real, dtype=torch.float64)
    for r in range(0, M, ROW_BLOCK):
        a = A[r:min(M, r + ROW_BLOCK), :n_real].double()
        S += a.t() @ B[r:min(M, r + ROW_BLOCK)][:, cols].double()
        if r < br:
            sb += a[:br - r].sum(0)
    return S, sb


def tn_reference(A, B, G0, b0, M, n_real, k_real, split_src, split_dst, bias_rows=0, alpha=1.0, factor=1.0, sums=None):
    """G0 + alpha * factor * A^T B in G's layout and b0 + alpha * factor * (column sums of the rows below bias_rows), f64.
    b0 None: no bias gradient.  sums: tn_sums of the same operands (the variants of a shape share them)."""
    S, sb = sums if sums is not None else tn_sums(A, B, M, n_real, k_real, split_src, split_dst, bias_rows)
    a = float(alpha) * float(factor)
    return G0.double() + a * S, (None if b0 is None else b0.double() + a * sb)


# ---------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    path: str                 # the kernel the SHAPE was chosen for: 't128' | 'phased'
    kid: int                  # ase_hip_gemm_tn_kernel_id
    shape: tuple              # (M, N, K, n_real, k_real, split_src, split_dst, bias_rows)
    store: str                # 'bf16' | 'f16' | 'f32' | 'x3' (ASE_F32X3)
    variant: str
    style: str = 'int'        # operands: 'int' small integers | 'wideA' / 'wideB' (x3: one side needs its lo part, the other has none)
    bias: bool = True
    alpha: float = 1.0
    factor: float = 0.0       # != 0: a scale record {factor, 0} rides as alpha_dev
    poison: bool = False

    @property
    def id(self):
        st = '' if self.style == 'int' else '-' + self.style
        return f'{self.path}-' + 'x'.join(str(v) for v in self.shape) + f'-{self.store}{st}-{self.variant}'


# (16-bit shape, the 4-byte shape or None): the smallest shapes that reach each path of the 128 x 128 kernel
T128 = [
    ((1, 8, 8, 1, 8, 8, 8, 0), (1, 4, 4, 1, 4, 4, 4, 0)),                      # one row, one output row, one chunk
    ((50, 128, 64, 100, 53, 37, 40, 0), (50, 128, 64, 100, 53, 37, 40, 0)),    # the concat gap inside a tile, ragged n_real
    # exactly one staged 16-bit tile, a second tile column 8 wide, bias_rows in the middle of a tile
    ((64, 136, 136, 130, 133, 100, 103, 37), (64, 132, 136, 130, 133, 100, 103, 37)),
    # several M-splits with a ragged last chunk, the gap ends on the tile boundary at 256, the bias limit inside a later split
    ((300, 64, 320, 48, 317, 253, 256, 200), (300, 64, 320, 48, 317, 253, 256, 200)),
    ((1000, 384, 384, 384, 384, 384, 384, 0), (1000, 384, 384, 384, 384, 384, 384, 0)),      # 9 tiles: the 512-workgroup branch
    ((16448, 128, 128, 128, 128, 128, 128, 0), (16448, 128, 128, 128, 128, 128, 128, 0)),    # dozens of splits into one tile
    ((131008, 304, 264, 300, 261, 253, 256, 65600), None),                     # one K-tile short of the phased threshold
]
PHASED = [
    (131072, 304, 264, 300, 261, 253, 256, 65600),       # ragged both ways (chunk-0 substitution), gap ends at 256, bias limit inside a split
    (32832, 1024, 1024, 1024, 1024, 1024, 1024, 0),      # 16 tiles, uneven m_chunk, a short last split
]
VARIANTS = [
    ('plain_bias', dict()),
    ('plain_nobias', dict(bias=False)),
    ('a4', dict(alpha=4.0)),
    ('a05_nobias', dict(alpha=0.5, bias=False)),
    ('scale_record', dict(factor=0.5)),
    ('poison', dict(poison=True)),
]
PHASED_VARIANTS = ('plain_bias', 'scale_record', 'poison')


def has_padding(shape):
    M, N, K, nr, kr, ss, sd, br = shape
    return nr < N or sd > ss or kr + (sd - ss) < K


def _variants(shape, names=None):
    for name, f in VARIANTS:
        if names is not None and name not in names:
            continue
        if f.get('poison') and not has_padding(shape):
            continue
        yield name, f


def cases():
    out = []
    for s16, s32 in T128:
        for name, f in _variants(s16):
            for store in ('bf16', 'f16'):
                out.append(Case('t128', 0, s16, store, name, **f))
        if s32 is not None:
            for name, f in _variants(s32):
                out.append(Case('t128', 0, s32, 'f32', name, **f))
                for style in ('wideA', 'wideB'):
                    out.append(Case('t128', 0, s32, 'x3', name, style=style, **f))
    for s in PHASED:
        for name, f in _variants(s, PHASED_VARIANTS):
            for store in ('bf16', 'f16'):
                out.append(Case('phased', 1, s, store, name, **f))
    return out


def kernel_id(lib, c, lda=None, ldb=None):
    M, N, K, nr, kr, ss, sd, br = c.shape
    pa, pb = pitch(c.store)
    return lib.ase_hip_gemm_tn_kernel_id(M, N, K, nr, br, lda or N + pa, ldb or K + pb, STORE_CODE[c.store])


# -------------------------------------------------------------------------------------------------------------------- builder
def bf16_lo(x):
    """The lo part of the ASE_F32X3 split: x - bf16(x) (exact in bf16 for the integers used here)."""
    return x - x.to(torch.bfloat16).to(x.dtype)


def _wide(shape, amax, g):
    """Integers of magnitude 257 .. amax, odd (so bf16 cannot hold them: the lo part is non-zero), random sign, some zeros."""
    v = torch.randint(128, (amax + 1) // 2, shape, generator=g) * 2 + 1
    v = v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    v[torch.rand(shape, generator=g) < 0.1] = 0
    return v.float()


def _narrow(shape, n, g):
    return torch.randint(-n, n + 1, shape, generator=g).float()


def operand_ranges(M, style):
    """(magnitude of A, magnitude of B).  'int': {-2 .. 2} from LARGE_M rows on, else {-16 .. 16}.  x3 styles: the wide side up to
    4095 (511 where the sums would leave 2^24), the narrow side up to 15 - as many as keep M * wide * narrow below 2^24 - 2^16."""
    if style == 'int':
        n = 2 if M >= LARGE_M else 16
        return n, n
    wide = 4095
    narrow = min(15, int((EXACT - 65536) // (M * 4104)))       # (|hi| + |lo| <= 4096 + 8)
    if narrow < 1:
        wide, narrow = 511, 1
    return (wide, narrow) if style == 'wideA' else (narrow, wide)


def _make_operands(shape, style, seed):
    """A [M, N], B [M, K] f32 with ZERO pad columns, G0 / b0 as integer counts (multiples of the launch's alpha later)."""
    M, N, K, nr, kr, ss, sd, br = shape
    g = torch.Generator().manual_seed(seed)
    na, nb = operand_ranges(M, style)
    cols = g_columns(kr, ss, sd)
    A, B = torch.zeros(M, N), torch.zeros(M, K)
    A[:, :nr] = _wide((M, nr), na, g) if style == 'wideA' else _narrow((M, nr), na, g)
    B[:, cols] = _wide((M, kr), nb, g) if style == 'wideB' else _narrow((M, kr), nb, g)
    G0 = torch.randint(1, 9, (nr, kr), generator=g).float() * (torch.randint(0, 2, (nr, kr), generator=g) * 2 - 1).float()
    b0 = torch.randint(1, 9, (nr,), generator=g).float() * (torch.randint(0, 2, (nr,), generator=g) * 2 - 1).float()
    sums = tn_sums(A, B, M, nr, kr, ss, sd, br)
    return A, B, G0, b0, sums


_OPERANDS = _LRU(3)


class Built:
    pass


def _holder(absA, absB):
    """Upper bound of max_{n,k} sum_m |A[m,n]| |B[m,k]| (the tighter side of Hoelder's inequality)."""
    return float(min(absA.sum(0).max() * absB.max(), absA.max() * absB.sum(0).max()))


def check_operands(A, B, shape, store, style, a, G0, b0, sums, bias):
    """The conditions the bitwise comparison of ONE problem rests on, and the ones that make it bite.  a = alpha * factor;
    G0 / b0 in units of a.  Returns the bound of sum |a| |b| (shared gradients add theirs)."""
    M, N, K, nr, kr, ss, sd, br = shape
    cols = g_columns(kr, ss, sd)
    Ar, Br = A[:, :nr], B[:, cols]
    S, sb = sums
    assert math.log2(a).is_integer(), 'alpha * factor is not a power of two'
    if store == 'x3':        # al*bh + ah*bl + ah*bh: exact only if one side has no lo part; every partial product sum is bounded
        la, lb = bf16_lo(Ar), bf16_lo(Br)
        wide, narrow = (la, lb) if style == 'wideA' else (lb, la)
        src = Ar if style == 'wideA' else Br
        assert style in ('wideA', 'wideB') and bool((narrow == 0).all()), 'x3: the narrow side has a lo part'
        assert bool((wide[src != 0] != 0).all()) and float((wide != 0).float().mean()) >= 0.5, 'x3: the wide side has no lo part'
        bound = _holder((Ar - la).abs() + la.abs(), (Br - lb).abs() + lb.abs())
    else:
        bound = _holder(Ar.abs(), Br.abs())
        if store in STORE_MAX:
            dt = STORE_DTYPE[store]
            assert float(Ar.abs().max()) <= STORE_MAX[store] and float(Br.abs().max()) <= STORE_MAX[store]
            assert torch.equal(Ar.to(dt).float(), Ar) and torch.equal(Br.to(dt).float(), Br)
    assert bound + float(G0.abs().max()) < EXACT, ('sum |a| |b| + |G0|', bound)
    assert bool((S == S.round()).all()) and float(S.abs().max()) <= bound
    bbound = float(Ar.abs().sum(0).max())
    if bias:
        assert bbound + float(b0.abs().max()) < EXACT, ('bias column sums', bbound)
    if M >= LARGE_M and style == 'int':
        assert float(Ar.abs().max()) <= 2 and float(Br.abs().max()) <= 2
    # ---- bite
    # (an operand with a handful of entries cannot hold a negative, a zero AND the non-zero entry the sums need: from 16 entries on
    #  each operand holds both, below that the two operands together do)
    for X in [X for X in (Ar, Br) if X.numel() >= 16] or [torch.cat([Ar.reshape(-1), Br.reshape(-1)])]:
        assert bool((X < 0).any()), 'no negative entries'
        assert bool((X == 0).any()), 'no zero entries'
    assert bool((torch.cat([Ar.reshape(-1), Br.reshape(-1)]) < 0).any()) and bool((torch.cat([Ar.reshape(-1), Br.reshape(-1)]) == 0).any())
    assert bool((G0 != 0).all()) and bool((b0 != 0).all()) and bool((G0 == G0.round()).all()) and bool((b0 == b0.round()).all())
    assert S.unique().numel() > 1, 'the sums are all equal'
    if bias and nr > 1:
        assert sb.unique().numel() > 1, 'the bias sums are all equal'
    if bias:
        assert bool((sb != 0).any())
    return bound


def _build(c, attempt):
    M, N, K, nr, kr, ss, sd, br = c.shape
    assert kr + (sd - ss) <= K and nr <= N
    seed = M * 7 + N * 3 + K + 1009 * nr + 100003 * attempt + {'int': 0, 'wideA': 1, 'wideB': 2}[c.style]
    A, B, G0, b0, sums = _OPERANDS.fetch((c.shape, c.style, seed), lambda: _make_operands(c.shape, c.style, seed))
    a = c.alpha * (c.factor or 1.0)
    assert math.log2(c.alpha).is_integer() and math.log2(c.factor or 1.0).is_integer()
    b = Built()
    b.case, b.A, b.B, b.a = c, A, B, a
    b.G0, b.b0 = G0 * a, (b0 * a if c.bias else None)                   # integer multiples of alpha * factor
    check_operands(A, B, c.shape, c.store, c.style, a, G0, b0, sums, c.bias)
    G, gb = tn_reference(A, B, b.G0, b.b0, M, nr, kr, ss, sd, br, alpha=c.alpha, factor=c.factor or 1.0, sums=sums)
    b.G, b.gb = G.float(), (None if gb is None else gb.float())
    assert torch.equal(b.G.double(), G) and (gb is None or torch.equal(b.gb.double(), gb)), 'the expected value is not exact in f32'
    assert not torch.equal(b.G, b.G0)
    return b


def build(c):
    """Operands + expected outputs of a case.  Tiny cases try further seeds until the conditions hold - the draw is still a
    function of the case alone; everything else must hold on its first draw."""
    M, N, K, nr, kr = c.shape[:5]
    tries = 64 if M * nr < 4096 else 1
    for attempt in range(tries):
        try:
            return _build(c, attempt)
        except AssertionError:
            if attempt == tries - 1:
                raise


# --------------------------------------------------------------------------------------------------------------------- runner
_DEVICE_OPERANDS = _LRU(2)


def pitch(store):
    """(lda - N, ldb - K): one / two 16-byte chunks."""
    e = 16 // torch.empty(0, dtype=STORE_DTYPE[store]).element_size()
    return e, 2 * e


def device_operands(A, B, shape, store, poison, dev):
    """A, B as views of larger NaN-filled buffers: NaN between the width and the pitch and in the rows after M; `poison` also in
    the pad columns the header names."""
    M, N, K, nr, kr, ss, sd, br = shape
    dt = STORE_DTYPE[store]
    pa, pb = pitch(store)
    nan = float('nan')
    Ab = torch.full((M + 3, N + pa), nan, dtype=dt)
    Bb = torch.full((M + 2, K + pb), nan, dtype=dt)
    Ab[:M, :N] = A.to(dt)
    Bb[:M, :K] = B.to(dt)
    if poison:
        Ab[:M, nr:N] = nan
        Bb[:M, ss:sd] = nan
        Bb[:M, kr + (sd - ss):K] = nan
    return Ab.to(dev)[:M, :N], Bb.to(dev)[:M, :K]


def windows(nr, kr, N, G0, b0, dev):
    """(G buffer, G window, gbias buffer, gbias window or None): the windows sit in longer flat sentinel buffers whose tails would
    take a whole stray row / every pad column's sum."""
    Gbuf = torch.full((G_BEFORE + nr * kr + 2 * kr + 5,), G_SENTINEL)
    Gbuf[G_BEFORE:G_BEFORE + nr * kr] = G0.reshape(-1)
    Gbuf = Gbuf.to(dev)
    Gw = Gbuf[G_BEFORE:G_BEFORE + nr * kr].view(nr, kr)
    if b0 is None:
        return Gbuf, Gw, None, None
    bbuf = torch.full((B_BEFORE + N + 6,), B_SENTINEL)
    bbuf[B_BEFORE:B_BEFORE + nr] = b0
    bbuf = bbuf.to(dev)
    return Gbuf, Gw, bbuf, bbuf[B_BEFORE:B_BEFORE + nr]


def check_windows(name, Gbuf, bbuf, nr, kr, G, gb):
    """Bitwise comparison of a gradient window and its bias window with the expected values, and of every sentinel around them.
    Returns (elements compared, elements not bitwise equal, sentinel words checked); raises on any difference."""
    got = Gbuf.cpu()
    w = got[G_BEFORE:G_BEFORE + nr * kr].view(nr, kr)
    diff = w.contiguous().view(torch.int32) != G.contiguous().view(torch.int32)
    n, bad = nr * kr, int(diff.sum())
    if bad:
        i = diff.nonzero()[0].tolist()
        raise AssertionError((name, 'G: elements not bitwise equal', bad, 'of', n, 'first (n, k)', i, 'got', float(w[i[0], i[1]]),
                              'want', float(G[i[0], i[1]])))
    edge = torch.cat([got[:G_BEFORE], got[G_BEFORE + nr * kr:]])
    assert bool((edge == G_SENTINEL).all()), (name, 'G: written outside [n_real, k_real]', int((edge != G_SENTINEL).sum()))
    sent = edge.numel()
    if bbuf is not None:
        s = bbuf.cpu()
        v = s[B_BEFORE:B_BEFORE + nr]
        badb = int((v.contiguous().view(torch.int32) != gb.contiguous().view(torch.int32)).sum())
        assert badb == 0, (name, 'gbias: elements not bitwise equal', badb, 'of', nr, 'got', v[:8].tolist(), 'want', gb[:8].tolist())
        edge = torch.cat([s[:B_BEFORE], s[B_BEFORE + nr:]])
        assert bool((edge == B_SENTINEL).all()), (name, 'gbias: written outside [n_real]', int((edge != B_SENTINEL).sum()))
        n, sent = n + nr, sent + edge.numel()
    return n, 0, sent


def launch_and_check(be, b, dev='cpu'):
    """One gemm_tn launch of a built case on backend `be` (HipBackend, or the emulator on the CPU) and the bitwise comparison.
    Returns (elements compared, elements not bitwise equal, sentinel words checked)."""
    c = b.case
    M, N, K, nr, kr, ss, sd, br = c.shape
    A, B = _DEVICE_OPERANDS.fetch((id(b.A), id(b.B), c.store, c.poison, str(dev)),
                                  lambda: device_operands(b.A, b.B, c.shape, c.store, c.poison, dev) + (b.A, b.B))[:2]
    Gbuf, Gw, bbuf, bw = windows(nr, kr, N, b.G0, b.b0, dev)
    rec = torch.tensor([c.factor, 0.0], dtype=torch.float32, device=dev) if c.factor else None
    be.gemm_tn(A, B, Gw, M, N, K, nr, kr, ss, sd, alpha=c.alpha, gbias=bw, bias_rows=br, alpha_dev=rec)
    out = check_windows(c.id, Gbuf, bbuf, nr, kr, b.G, b.gb)
    if rec is not None:
        r = rec.cpu()
        assert float(r[0]) == c.factor and r[1:].view(torch.int32).item() == 0, (c.id, 'the scale record was written')
    return out


# -------------------------------------------------------------------------------------------------------------------- grouped
# a problem: (shape, owner) - owner = index of the problem whose G / gbias it adds into (itself: a gradient of its own)
TILES_WIDTHS = [(8, 8, 8, 8, 8, 8, 0), (264, 136, 257, 133, 100, 103, 64)]


def group_sets():
    """name -> (problems, target_wg).  'tiles': 1 to 4 K-tiles per work item (the nk == 1 prologue, the all-tail loops, the first
    steady-state iteration) on a narrow and a ragged width (n_real = 257: the second n-tile has one live row).  'splits': several
    splits per tile (asserted on the plan's reduce table), the bias limit inside a split.  'shared': two problems with different
    operands and M add into the SAME G / gbias (the planner sets bit 30), a third owns its own."""
    tiles = [((M,) + w, None) for w in TILES_WIDTHS for M in (64, 128, 192, 256)]
    splits = [((1280, 304, 320, 300, 317, 253, 256, 768), None)]
    shared = [((128, 264, 136, 257, 133, 100, 103, 64), None), ((320, 264, 136, 257, 133, 100, 103, 128), 0),
              ((64, 136, 264, 130, 261, 253, 256, 0), None)]

    def own(ps, base=0):
        return [(s, (i if o is None else o) + base) for i, (s, o) in enumerate(ps)]
    sets = {'tiles': (own(tiles), 0), 'splits': (own(splits), 8), 'shared': (own(shared), 0)}
    sets['all'] = (own(tiles) + own(splits, len(tiles)) + own(shared, len(tiles) + len(splits)), 8)
    return sets


class BuiltGroup:
    pass


_GROUP_OPERANDS = _LRU(4)


def build_group(name, store, alpha=1.0, factor=0.0, poison=False):
    """Operands, initial and expected gradients of a set.  Every problem has operands of its own; a gradient's expected value adds
    the sums of every problem that owns it, and the exactness bound is the sum of theirs."""
    problems, target_wg = group_sets()[name]
    a = alpha * (factor or 1.0)
    g = BuiltGroup()
    g.name, g.store, g.alpha, g.factor, g.poison, g.target_wg, g.a = name, store, alpha, factor, poison, target_wg, a
    g.problems, g.ops, g.grads = problems, [], {}
    bounds = {}
    for i, (shape, owner) in enumerate(problems):
        M, N, K, nr, kr, ss, sd, br = shape
        assert M % 64 == 0 and br % 64 == 0
        seed = 5000011 + 131 * i + M * 7 + N * 3 + K
        A, B, G0, b0, sums = _GROUP_OPERANDS.fetch((shape, seed), lambda: _make_operands(shape, 'int', seed))
        bound = check_operands(A, B, shape, store, 'int', a, G0, b0, sums, True)
        g.ops.append((A, B))
        if owner == i:
            g.grads[i] = [G0 * a, b0 * a, (G0 * a).double(), (b0 * a).double()]          # G0, b0, expected G, expected gbias
            bounds[i] = bound + float(G0.abs().max())
        else:
            assert problems[owner][0][3:7] == shape[3:7] and problems[owner][1] == owner
            bounds[owner] += bound
        e = g.grads[owner]
        e[2], e[3] = tn_reference(A, B, e[2], e[3], M, nr, kr, ss, sd, br, alpha=alpha, factor=factor or 1.0, sums=sums)
    assert max(bounds.values()) < EXACT
    for e in g.grads.values():
        assert torch.equal(e[2].float().double(), e[2]) and torch.equal(e[3].float().double(), e[3])
        e[2], e[3] = e[2].float(), e[3].float()
    return g


def host_plan(lib, problems, target_wg):
    """The host-only planner on a table with made-up addresses (gradients that share an owner share theirs) -> (reduce table
    [(problem, tile, first slab, splits)], field 15 of every problem).  No GPU needed."""
    n = len(problems)
    tab = (ctypes.c_int64 * (16 * n))()
    for i, (shape, owner) in enumerate(problems):
        M, N, K, nr, kr, ss, sd, br = shape
        row = [0x100000 + i * 0x1000, N, 0x200000 + i * 0x1000, K, 0x40000000 + owner * 0x100000, 0x50000000 + owner * 0x1000,
               br, M, N, K, nr, kr, ss, sd, struct.unpack('<i', struct.pack('<f', 1.0))[0], 0]
        for j, v in enumerate(row):
            tab[16 * i + j] = v
    work, red = (ctypes.c_int32 * (4 * 8192))(), (ctypes.c_int32 * (4 * 8192))()
    nw, nr_ = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.ase_hip_gemm_tn_grouped_plan(tab, n, target_wg, work, 8192, ctypes.byref(nw), red, 8192, ctypes.byref(nr_))
    assert rc == 0, lib.ase_hip_last_error()
    return [tuple(red[4 * i:4 * i + 4]) for i in range(nr_.value)], [tab[16 * i + 15] for i in range(n)]


def launch_group_and_check(be, g, dev='cpu'):
    """One grouped launch of a built set (HipBackend with or without its workspace, or the emulator) and the bitwise comparison of
    every gradient window.  Returns (plan, elements compared, elements not bitwise equal, sentinel words checked)."""
    bufs, probs = {}, []
    for i, (shape, owner) in enumerate(g.problems):
        M, N, K, nr, kr, ss, sd, br = shape
        if owner == i:
            bufs[i] = windows(nr, kr, N, g.grads[i][0], g.grads[i][1], dev)
    for i, (shape, owner) in enumerate(g.problems):
        M, N, K, nr, kr, ss, sd, br = shape
        A, B = device_operands(g.ops[i][0], g.ops[i][1], shape, g.store, g.poison, dev)
        _, Gw, _, bw = bufs[owner]
        probs.append((A, B, Gw, bw, br, M, N, K, nr, kr, ss, sd, g.alpha))
    rec = torch.tensor([g.factor, 0.0], dtype=torch.float32, device=dev) if g.factor else None
    plan = be.make_tn_plan(probs, g.target_wg, alpha_dev=rec)
    be.gemm_tn_grouped(plan)
    n = bad = sent = 0
    for i, (Gbuf, Gw, bbuf, bw) in bufs.items():
        nr, kr = g.problems[i][0][3:5]
        r = check_windows(f'{g.name}-{g.store}-problem{i}', Gbuf, bbuf, nr, kr, g.grads[i][2], g.grads[i][3])
        n, bad, sent = n + r[0], bad + r[1], sent + r[2]
    if rec is not None:
        r = rec.cpu()
        assert float(r[0]) == g.factor and r[1:].view(torch.int32).item() == 0, (g.name, 'the scale record was written')
    return plan, n, bad, sent
