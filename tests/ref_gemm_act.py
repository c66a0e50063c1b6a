"""f64 reference of ase_hip_gemm_nt's activation family, its data-gradient epilogue and its non-finite contract - TEST
INFRASTRUCTURE ONLY (CPU, torch).  Written from include/ase_hip.h ("Dense layers") and torch.nn.functional, not from the emulator
or the kernels' act.h.

The idea is tests/ref_gemm.py's: integer operands, a power-of-two alpha (and record factor) make alpha * A.B^T EXACT in f32 in any
summation order, so the pre-activation is one known f32 number, z = RN_f32(alpha P + bias) - whether or not the compiler fuses the
multiply-add, because the product is exact and only the sum rounds.  Everything a launch stores is then a function of a known z:
the matrix product contributes no error and hides none.

  forward   stored = conversion of act(z):  ref64 = F.<act>(z.double()),  e_ref = |F.<act>(z) in f32 on the CPU - ref64|
  z twin    (act >= SILU, mask_out)  BITWISE the storage conversion of z (f16 saturating, as ref_gemm.nt_store)
  bit twin  (ACT_TANH, mask_out)  bit = (stored C > 0) on the values read back; bit = sign of ref64 wherever |ref64| > allowance
  colsum    the f64 column sums of the values the launch STORED, within depth x 2^-24 x sum |stored| (see DEPTH)
  backward  ASE_AUX_PREACT | act << 8:  stored = conversion of (alpha P) act'(a), a = the aux operand as stored;  ref64 / e_ref from
            autograd of F.<act> at a.double() / a.float().  ACT_TANH's backward is ASE_AUX_TANH_GRAD on the tanh OUTPUT: (alpha P) (1 - a^2).

BOUND (ref_heads.within) per BAND of z (of a for the backward), so that a large value cannot pay for a small one
- softplus(-20) = 2e-9 is not judged against max |ref| = 30:
      max |got - ref64| <= 2 e_ref + 2^-23 max |ref64| + TINY + half a storage ulp        (e_ref, max over the band)
  bands [-30, -8), [-8, -1), [-1, 1], (1, 8], (8, 30], and the two outer bands beyond +-30 that the operands' tails reach; PLANTED
  elements (a zero row of A over a planted bias column: z = the planted value exactly) are compared ONE BY ONE.
  TINY = 2^-126, the smallest normal f32: f32 arithmetic has an absolute floor as well as a relative one - a result below it (sigmoid(-88.8)
  = 2.7e-39, SiLU(-104) = -7e-44) may be flushed to +-0 by any of the f32 operations that form it, on the CPU or the device.  In the
  backward the factor act'(a) may flush before it meets the upstream gradient, so the floor there is TINY (1 + |alpha P|).
  Non-finite entries are equal as such.

DEPTH of a column sum, counted from the LDS-slab epilogue (csrc/gemm_nt_kernels.h nt_epilogue_impl; every colsum launch takes it):
a wave handles its sub-tile in chunks of FMC x 32 rows by FNC x 32 columns, a lane owning 4 columns and every (64 / (8 FNC))-th row
of the chunk.  Per chunk and column: NIT = FMC x 32 / (64 / (8 FNC)) additions down the lane's rows, log2(64 / (8 FNC)) __shfl_xor
steps across the lanes that share the column, then ONE atomic addition into colsum.  The atomics of a column - one per 32 FMC rows
of the grid's padded row range, ceil(M / BM) x BM / (32 FMC), rows past M adding 0 - follow each other onto the running total, so
the longest path a stored value takes is NIT + log2(64 / (8 FNC)) + that many f32 additions, each rounding at half an ulp of a partial
sum no larger than sum |term|:  |error| <= depth 2^-24 (sum |stored| + |initial value|)  (ref_heads.bias_within's rule).
SLAB_TILE lists (BM, FMC, FNC) per kernel id from dispatch_nt's instantiations.
"""
import math
from dataclasses import dataclass, replace
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from ase_amd.lib import (ACT_ELU, ACT_GELU, ACT_NONE, ACT_RELU, ACT_SELU, ACT_SIGMOID, ACT_SILU, ACT_SOFTPLUS, ACT_TANH, AUX_NONE,
                         AUX_PREACT, AUX_TANH_GRAD, BF16, F16, F32, F32H3, F32X3)
from tests import ref_gemm as R
from tests.ref_heads import half_ulp

TINY = 2.0 ** -126
F16_MAX = R.F16_MAX
ACT_NAME = {ACT_NONE: 'none', ACT_RELU: 'relu', ACT_TANH: 'tanh', ACT_SILU: 'silu', ACT_ELU: 'elu', ACT_GELU: 'gelu',
            ACT_SIGMOID: 'sigmoid', ACT_SELU: 'selu', ACT_SOFTPLUS: 'softplus'}
# torch.nn.functional with the header's parameters: ELU alpha 1, exact-erf GELU, Softplus beta 1 / threshold 20
ACT_FN = {ACT_TANH: torch.tanh, ACT_SILU: F.silu, ACT_ELU: lambda z: F.elu(z, alpha=1.0),
          ACT_GELU: lambda z: F.gelu(z, approximate='none'), ACT_SIGMOID: torch.sigmoid, ACT_SELU: F.selu,
          ACT_SOFTPLUS: lambda z: F.softplus(z, beta=1.0, threshold=20.0), ACT_RELU: torch.relu, ACT_NONE: lambda z: z}
SMOOTH = (ACT_SILU, ACT_ELU, ACT_GELU, ACT_SIGMOID, ACT_SELU, ACT_SOFTPLUS)
ACTS = (ACT_TANH,) + SMOOTH
BANDS = ('[-inf,-30)', '[-30,-8)', '[-8,-1)', '[-1,1]', '(1,8]', '(8,30]', '(30,inf]')
INNER = BANDS[1:6]
PLANTED = (0.0, 20.0, float(torch.nextafter(torch.tensor(20.0), torch.tensor(math.inf))), 100.0, -100.0, 88.8, -88.8, -104.0,
           1e-3, -1e-3)
F16_PLANT = 70000.0            # one more column (f16, ACT_SIGMOID, a record): act(z) = 1 is finite, the twin saturates


def act_grad(act, a, dtype):
    """act'(a) by autograd of the torch activation, evaluated in `dtype`."""
    x = a.to(dtype).detach().clone().requires_grad_(True)
    ACT_FN[act](x).sum().backward()
    return x.grad


def band_index(z):
    """Index into BANDS of every element of z (f32 / f64)."""
    z = z.double()
    idx = torch.full(z.shape, 3, dtype=torch.int64)          # [-1, 1]
    idx[z < -1.0] = 2
    idx[z < -8.0] = 1
    idx[z < -30.0] = 0
    idx[z > 1.0] = 4
    idx[z > 8.0] = 5
    idx[z > 30.0] = 6
    return idx


def planted_columns(N):
    """len(PLANTED) distinct columns: the first ones, those either side of the first 32-column fragment boundary, the last valid ones."""
    cols = sorted({0, 1, 2, 29, 30, 31, 32, 33, N - 2, N - 1})
    assert len(cols) == len(PLANTED) and N >= 36
    return cols


# ---------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    kid: int
    M: int
    N: int
    K: int
    store: str                # as ref_gemm: 'bf16' | 'f16' | 'f32' | 'x3' | 'h3'
    act: int
    variant: str
    back: bool = False        # the data-gradient launch (ASE_AUX_PREACT | act << 8, ASE_AUX_TANH_GRAD for tanh) instead of the forward
    twin: bool = False        # forward: mask_out present (the z twin; ACT_TANH: the bit matrix, N % 32 == 0)
    colsum_n: int = 0
    out_f32: bool = False
    alpha: float = 1.0
    factor: float = 0.0       # != 0: a scale record {factor, 0}
    stacked: bool = False
    f16_plant: bool = False
    exps: tuple = None

    @property
    def id(self):
        return f'k{self.kid}-{self.M}x{self.N}x{self.K}-{self.store}-{ACT_NAME[self.act]}-{self.variant}'

    @property
    def out_dtype(self):
        return torch.float32 if self.out_f32 else R.STORE_DTYPE[self.store]


SMALL_16 = [(0, (70, 36, 32)), (1, (130, 132, 32)), (5, (130, 132, 64))]
SMALL_32 = [(0, (70, 36, 16)), (1, (130, 132, 48)), (5, (130, 132, 32))]
# once per remaining slab instantiation (SiLU - non-monotonic - and tanh only): the shapes row a9k found to be the smallest per leaf
LARGE_16 = [(1, (16300, 516, 64)), (4, (8200, 452, 64)), (2, (32700, 512, 64)), (2, (65536, 256, 64)), (6, (49000, 256, 64))]
LARGE_32 = [(1, (16300, 516, 32)), (4, (8200, 452, 32)), (3, (49000, 256, 32))]


def _small_variants(N, act, sixteen):
    tw = act != ACT_TANH or N % 32 == 0          # tanh's twin is the bit matrix
    v = [('fwd', dict()), ('fwd_colsum_n', dict(colsum_n=N, twin=tw)), ('fwd_colsum_n5', dict(colsum_n=N - 5)),
         ('fwd_a05_rec', dict(alpha=0.5, factor=0.5, twin=tw)),
         ('bwd', dict(back=True)), ('bwd_a05_rec', dict(back=True, alpha=0.5, factor=0.5)),
         ('bwd_colsum_n5', dict(back=True, colsum_n=N - 5)), ('bwd_stacked', dict(back=True, stacked=True))]
    if tw:
        v.insert(1, ('fwd_twin', dict(twin=True)))
    if sixteen:
        v += [('fwd_out_f32', dict(out_f32=True, twin=tw)), ('bwd_out_f32', dict(back=True, out_f32=True))]
    return v


def cases():
    out = []
    for shapes, stores in ((SMALL_16, ('bf16', 'f16')), (SMALL_32, ('f32', 'x3', 'h3'))):
        for kid, (M, N, K) in shapes:
            for store in stores:
                for act in ACTS:
                    for name, f in _small_variants(N, act, store in ('bf16', 'f16')):
                        out.append(Case(kid, M, N, K, store, act, name, **f))
                if store == 'f16':               # the saturating twin and its overflow report
                    out.append(Case(kid, M, N, K, store, ACT_SIGMOID, 'fwd_twin_rec', twin=True, factor=1.0))
                    out.append(Case(kid, M, N, K, store, ACT_SIGMOID, 'fwd_twin_rec_70000', twin=True, factor=1.0, f16_plant=True))
    for shapes, stores in ((LARGE_16, ('bf16', 'f16')), (LARGE_32, ('f32', 'x3', 'h3'))):
        for kid, (M, N, K) in shapes:
            for store in stores:
                for act in (ACT_SILU, ACT_TANH):
                    out.append(Case(kid, M, N, K, store, act, 'fwd_twin', twin=act != ACT_TANH or N % 32 == 0))
                    out.append(Case(kid, M, N, K, store, act, 'bwd', back=True))
    return out


def shapes():
    """[(M, N, K, dtype code, kernel id)] for the check against ase_hip_gemm_nt_kernel_id."""
    out = []
    for lst, codes in ((SMALL_16 + LARGE_16, (BF16, F16)), (SMALL_32 + LARGE_32, (F32, F32X3, F32H3))):
        out += [(M, N, K, code, kid) for kid, (M, N, K) in lst for code in codes]
    return out


# -------------------------------------------------------------------------------------------------------------------- builder
_OPS, _Z = R._LRU(3), R._LRU(4)


def _spread(a):
    """Target standard deviation of A.B^T for which z = a P + bias spreads over the bands: sigma(z) of about 10."""
    return 10.0 / a


def _operands(M, N, K, a, attempt):
    n = R.operand_range(SimpleNamespace(spread=_spread(a) * (1.0 + 0.5 * attempt), K=K))
    seed = M * 7 + N * 3 + K + 100003 * attempt
    return _OPS.fetch((M, N, K, n, seed), lambda: R._make_operands(M, N, K, n, seed, False)) + (n,)


def _z(c, attempt):
    """(A, B, bias with the planted entries, aP f32 [M, N] = alpha' A.B^T (exact), z f32 = RN(aP + bias), planted mask, n)."""
    a = c.alpha * (c.factor or 1.0)
    A, B, bias, P, bound, n = _operands(c.M, c.N, c.K, a, attempt)

    def make():
        b = bias.clone()
        cols = planted_columns(c.N)
        shift = c.act % len(PLANTED)               # every value meets the fragment boundary under some activation
        for i, col in enumerate(cols):
            b[col] = PLANTED[(i + shift) % len(PLANTED)]
        if c.f16_plant:
            b[3] = F16_PLANT
        aP64 = P * a
        aP = aP64.float()
        assert math.log2(a).is_integer() and bound < R.EXACT and a * bound < R.EXACT
        assert bool((aP.double() == aP64).all()), 'alpha A.B^T is not exact in f32'
        z = (aP64 + b.double()).float()            # ONE rounding (f64 holds the sum of two f32 numbers this close exactly)
        zero_rows = (A == 0).all(1)
        planted = torch.zeros(c.M, c.N, dtype=torch.bool)
        planted[zero_rows.nonzero()[:, None], torch.tensor(cols)[None, :]] = True
        if c.f16_plant:
            planted[zero_rows, 3] = True
        assert bool(zero_rows.any()) and bool((z[planted].double().unsqueeze(1) == b.double()[None, :]).any(1).all())
        return b, aP, z, planted
    b, aP, z, planted = _Z.fetch((c.M, c.N, c.K, a, c.act % len(PLANTED), c.f16_plant, attempt), make)
    return A, B, b, aP, z, planted, n


def _build(c, attempt):
    assert c.act in ACTS and not (c.f16_plant and (c.store != 'f16' or c.act != ACT_SIGMOID or not c.factor))
    A, B, bias, aP, z, planted, n = _z(c, attempt)
    b = SimpleNamespace()
    b.case, b.A, b.B, b.n = c, A, B, n
    b.bias = None if c.back else bias
    b.aux, b.aux_mode, b.aux_split, b.aux_delta = None, AUX_NONE, 0, 0
    dt = R.STORE_DTYPE[c.store]
    b.extra = None
    if not c.back:
        b.arg, b.planted = z, planted
        b.ref32 = ACT_FN[c.act](z)
        b.ref64 = ACT_FN[c.act](z.double())
        b.twin = R.nt_store(z, dt)[0] if (c.twin and c.act != ACT_TANH) else None
    else:
        # the mask operand: what the forward of the same layer leaves as its twin - z (tanh: tanh(z)) in the storage type - moved down
        # one row, so that the planted values (zero rows of A, where the upstream gradient alpha P would be 0 too) meet ordinary rows
        src = torch.tanh(z) if c.act == ACT_TANH else z
        aux = R.nt_store(torch.roll(src, 1, 0), dt)[0]
        pl, zsrc = torch.roll(planted, 1, 0), torch.roll(z, 1, 0)
        if c.stacked:
            b.aux_split, b.aux_delta = R.stacked_rows(c.M)
            rows = torch.arange(c.M)
            rows = torch.where(rows >= b.aux_split, rows - b.aux_delta, rows)
            used, pl, zsrc = aux[rows], pl[rows], zsrc[rows]
            aux = aux.clone()
            aux[b.aux_split:] = 3.0                # rows no valid m maps to
        else:
            used = aux
        b.aux, b.aux_mode = aux, (AUX_TANH_GRAD if c.act == ACT_TANH else AUX_PREACT | (c.act << 8))
        a32, a64 = used.float(), used.double()
        if c.act == ACT_TANH:
            g32, g64 = 1.0 - a32 * a32, 1.0 - a64 * a64
        else:
            g32, g64 = act_grad(c.act, a32, torch.float32), act_grad(c.act, a64, torch.float64)
        # (bands by the operand; tanh's operand is its OUTPUT, all of it in [-1, 1]: its bands are those of the z behind it)
        b.arg, b.planted = (zsrc if c.act == ACT_TANH else a32), pl & (aP != 0)
        b.ref32, b.ref64 = aP * g32, aP.double() * g64
        b.twin = None
        b.extra = TINY * aP.double().abs()         # act'(a) below the smallest normal f32 may flush BEFORE the product with alpha P
    b.band = band_index(b.arg)
    b.band[b.planted] = -1
    # ---- the fixture conditions (retry other operand ranges, never a weaker condition)
    counts = torch.bincount(b.band[b.band >= 0].flatten(), minlength=len(BANDS))
    b.band_counts = counts
    assert all(int(counts[i]) >= 64 for i in range(1, 6)), ('a band holds fewer than 64 elements', counts.tolist())
    assert float((z < 0).float().mean()) >= 0.10, 'fewer than 10 % of z negative'
    assert int(b.planted.sum()) >= len(PLANTED), 'the planted values are not all there'
    assert bool(torch.isfinite(b.ref64).all()) and float(b.ref64.abs().max()) < F16_MAX
    if c.out_dtype != torch.float32:
        b.rounded = float((b.ref32.to(c.out_dtype).float() != b.ref32).float().mean())
        assert b.rounded >= 0.05, ('fewer than 5 % of the outputs are changed by the conversion', b.rounded)
    if c.store == 'h3':
        assert n * 2.0 ** c.exps[0] < F16_MAX and n * 2.0 ** c.exps[1] < F16_MAX
    if c.f16_plant:
        assert float(z[b.planted & (z == F16_PLANT)].numel()) >= 1
    return b


def build(c):
    if c.store == 'h3' and not c.exps:
        c = replace(c, exps=(12, 11))              # operands of a few units: far inside half's range at the largest scales
    for attempt in range(6):
        try:
            return _build(c, attempt)
        except AssertionError:
            if attempt == 5:
                raise


# ---------------------------------------------------------------------------------------------------------------------- bound
def allowance(ref64, ref32, band, storage, extra=None):
    """Elementwise tolerance of the module docstring's rule: per band, the band's e_ref and max |ref64|; band -1 (planted) one by
    one.  Returns (tolerance before the storage ulp, tolerance, e_ref per element's band)."""
    d = (ref32.double() - ref64).abs()
    e_ref, big = d.clone(), ref64.abs().clone()
    for i in range(len(BANDS)):
        m = band == i
        if bool(m.any()):
            e_ref[m] = d[m].max()
            big[m] = ref64[m].abs().max()
    base = 2.0 * e_ref + 2.0 ** -23 * big + TINY
    if extra is not None:
        base = base + extra
    return base, base + half_ulp(ref64.abs() + base, storage), e_ref


def check_values(got, b, name, report=None, storage=None):
    """`got` (the stored C, any dtype) against the built case under the rule; fills report[(act, store, direction)] with the observed
    maximum per band and its e_ref.  Raises AssertionError with the figures."""
    c = b.case
    storage = c.out_dtype if storage is None else storage
    got = got.double()
    r64 = b.ref64.clamp(-F16_MAX, F16_MAX) if storage == torch.float16 else b.ref64
    base, tol, e_ref = allowance(r64, b.ref32, b.band, storage, b.extra)
    assert bool(torch.isfinite(got).all()), (name, 'non-finite values stored', int((~torch.isfinite(got)).sum()))
    err = (got - r64).abs()
    worst = {}
    for i in list(range(len(BANDS))) + [-1]:
        m = b.band == i
        if bool(m.any()):
            worst['planted' if i < 0 else BANDS[i]] = (float(err[m].max()), float(e_ref[m].max()), float(tol[m].max()))
    if report is not None:
        key = (ACT_NAME[c.act], 'bwd' if c.back else 'fwd', str(storage).replace('torch.', ''))
        cur = report.setdefault(key, {})
        for k, (e, r, t) in worst.items():
            if k not in cur or e > cur[k][0]:
                cur[k] = (e, r, t)
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.argmax((err - tol).flatten()))
        m, n = divmod(i, c.N)
        raise AssertionError((name, 'outside the bound', int(bad.sum()), 'of', got.numel(), 'worst (m, n)', (m, n), 'argument',
                              float(b.arg[m, n]), 'got', float(got[m, n]), 'ref64', float(r64[m, n]), 'err', float(err[m, n]),
                              'tol', float(tol[m, n]), 'e_ref', float(e_ref[m, n]), 'planted' if b.band[m, n] < 0 else BANDS[b.band[m, n]]))
    return worst


# --------------------------------------------------------------------------------------------------------------------- runner
C_SENTINEL, CS_INIT, TWIN_SENTINEL = R.C_SENTINEL, R.CS_INIT, -11.0
_DEV = R._LRU(2)


def _device_operands(be, b, dev):
    c = b.case
    dt = R.STORE_DTYPE[c.store]
    pad = 16 // torch.empty(0, dtype=dt).element_size()

    def make():
        A = R._padded(b.A, dt, pad, dev)
        if c.store == 'h3':
            B = torch.zeros(c.N, c.K, dtype=dt, device=dev)
            be.refresh_shadow(b.B.to(dev), B, None, c.K, c.K, x3_exp=c.exps[1])
        else:
            B = R._padded(b.B, dt, 2 * pad, dev)
        return A, B, b.A, b.B
    return _DEV.fetch((id(b.A), id(b.B), c.store, c.exps, str(dev)), make)[:2]


def _edges_intact(buf, M, N, off, sentinel, name):
    for what, edge in (('rows after M', buf[M:]), ('columns before', buf[:M, :off]), ('columns after N', buf[:M, off + N:])):
        assert bool((edge == sentinel).all()), (name, 'written outside [M, N]', what)


def launch(be, b, dev='cpu', A=None, bias=None, act=None, colsum_n=None, twin=None, record=None):
    """One gemm_nt launch of a built case into views of larger sentinel-filled buffers: ldc > N with a column offset, ldmask > N
    with a column offset for the twin, lda / ldb / ldaux padded, rows after M - every sentinel checked before returning.
    Returns a namespace: C [M, N], twin [M, N] (z twin) or words [M, N / 32] (bit twin) or None, colsum f32 [colsum_n] or None,
    rec f32 [2] or None - all on the CPU.  The keyword arguments override the case (the non-finite tests reuse this runner)."""
    c = b.case
    M, N, K = c.M, c.N, c.K
    dt = R.STORE_DTYPE[c.store]
    pad = 16 // torch.empty(0, dtype=dt).element_size()
    act = (ACT_NONE if c.back else c.act) if act is None else act      # (the data-gradient launch has no activation of its own)
    colsum_n = c.colsum_n if colsum_n is None else colsum_n
    twin = c.twin if twin is None else twin
    record = (c.factor or None) if record is None else (record or None)
    kw = {'x3_exps': c.exps} if c.store == 'h3' else {}
    Ad, Bd = _device_operands(be, b, dev)
    if A is not None:
        Ad = R._padded(A, dt, pad, dev)
    bias = b.bias if bias is None else bias
    Cbuf = torch.full((M + 3, N + 24), C_SENTINEL, dtype=c.out_dtype, device=dev)
    Tbuf = Tm = cbuf = rec = aux = None
    smooth = act >= ACT_SILU
    if twin and not c.back:
        if smooth:
            Tbuf = torch.full((M + 2, N + 24), TWIN_SENTINEL, dtype=dt, device=dev)
            Tm = Tbuf[:M, 8:8 + N]
        else:
            Tbuf = torch.full((M + 2, N // 32 + 3), R.BITS_SENTINEL, dtype=torch.int32, device=dev)
            Tm = Tbuf[:M, 1:1 + N // 32]
    if colsum_n > 0:
        cbuf = torch.full((colsum_n + 13,), CS_INIT, dtype=torch.float32, device=dev)
    if record:
        rec = torch.tensor([record, 0.0], dtype=torch.float32, device=dev)
    if b.aux is not None:
        aux = R._padded(b.aux, dt, pad, dev)
    be.gemm_nt(Ad, Bd, Cbuf[:M, 8:8 + N], M, N, K, bias=None if bias is None else bias.to(dev), aux=aux, aux_mode=b.aux_mode,
               colsum=None if cbuf is None else cbuf[4:], colsum_n=colsum_n, act=act, alpha=c.alpha,
               aux_split=b.aux_split, aux_delta=b.aux_delta, mask_out=Tm, alpha_dev=rec, **kw)
    out = SimpleNamespace(twin=None, colsum=None, rec=None)
    got = Cbuf.cpu()
    _edges_intact(got, M, N, 8, C_SENTINEL, (c.id, 'C'))
    out.C = got[:M, 8:8 + N]
    if Tbuf is not None:
        t = Tbuf.cpu()
        if smooth:
            _edges_intact(t, M, N, 8, TWIN_SENTINEL, (c.id, 'twin'))
            out.twin = t[:M, 8:8 + N]
        else:
            _edges_intact(t, M, N // 32, 1, R.BITS_SENTINEL, (c.id, 'mask_out'))
            out.twin = t[:M, 1:1 + N // 32]
    if cbuf is not None:
        s = cbuf.cpu()
        assert bool((s[:4] == CS_INIT).all()) and bool((s[4 + colsum_n:] == CS_INIT).all()), (c.id, 'colsum: written outside [0, colsum_n)')
        out.colsum = s[4:4 + colsum_n]
    if rec is not None:
        out.rec = rec.cpu()
    return out


# kernel id -> (tile rows BM, FMC, FNC) of the slab epilogue that id's colsum launches run (csrc/gemm_nt_kernels.h dispatch_nt:
# launch_nt<T, WGM, WGN, FM, FN, ..> has BM = WGM FM 32 and calls nt_epilogue<T, FM, FN, FMC = FM, FNC = min(FN, 2)>; 16-bit ids 2 / 6
# fall back to launch_nt8<T, false>: 256-row tiles, nt_epilogue<T, 4, 2, 2, 2>)
SLAB_TILE = {0: (64, 1, 1), 1: (128, 2, 2), 2: (256, 2, 2), 3: (256, 2, 2), 4: (64, 1, 2), 5: (64, 1, 1), 6: (256, 2, 2)}


def colsum_depth(kid, M):
    """f32 additions on the longest path of a column sum (module docstring, DEPTH)."""
    BM, FMC, FNC = SLAB_TILE[kid]
    lanes_per_row = 8 * FNC
    rows_per_step = 64 // lanes_per_row
    nit = FMC * 32 // rows_per_step
    atomics = -(-M // BM) * BM // (32 * FMC)
    return nit + int(math.log2(rows_per_step)) + atomics


def check_colsum(colsum, stored, colsum_n, name, kid, report=None, key=None):
    """The column sums against the f64 sums of what the launch stored (+ the buffer's initial value), within DEPTH (module
    docstring).  Returns the largest error / allowance and notes it in report[key]."""
    s = stored.double()[:, :colsum_n]
    want = s.sum(0) + CS_INIT
    depth = colsum_depth(kid, stored.shape[0])
    tol = depth * 2.0 ** -24 * (s.abs().sum(0) + CS_INIT)
    err = (colsum.double() - want).abs()
    ratio = float((err / tol).max())
    if report is not None:
        cur = report.setdefault(key, {'error / allowance': 0.0})
        if ratio >= cur['error / allowance']:
            cur.update({'error / allowance': ratio, 'error': float(err.max()), 'depth': depth, 'rows': stored.shape[0]})
    assert bool((err <= tol).all()), (name, 'colsum', float(err.max()), 'allowed', float(tol[err.argmax()]), 'depth', depth)
    return ratio


def launch_and_check(be, b, dev='cpu', report=None):
    """Launch a built case and hold everything it stored to the reference.  Returns the number of elements compared."""
    c = b.case
    o = launch(be, b, dev)
    check_values(o.C, b, c.id, report)
    n = c.M * c.N
    if c.twin and not c.back:
        if c.act == ACT_TANH:
            bits = R.unpack_bits(o.twin, c.N)
            assert torch.equal(bits, o.C.float() > 0), (c.id, 'mask_out bit != (stored C > 0)', int((bits != (o.C.float() > 0)).sum()))
            base = allowance(b.ref64, b.ref32, b.band, c.out_dtype, b.extra)[1]
            sure = b.ref64.abs() > base
            assert torch.equal(bits[sure], (b.ref64 > 0)[sure]), (c.id, 'mask_out bit != sign of the reference')
        else:
            if not torch.equal(o.twin, b.twin):
                bad = (o.twin != b.twin).nonzero()
                raise AssertionError((c.id, 'z twin not bitwise the conversion of z', len(bad), 'first (m, n)', bad[0].tolist(),
                                      'got', float(o.twin[bad[0, 0], bad[0, 1]]), 'want', float(b.twin[bad[0, 0], bad[0, 1]])))
        n += c.M * c.N
    if c.colsum_n > 0:
        check_colsum(o.colsum, o.C, c.colsum_n, c.id, c.kid, report, ('colsum', str(c.out_dtype).replace('torch.', ''), f'k{c.kid}'))
        n += c.colsum_n
    if o.rec is not None:
        assert float(o.rec[0]) == c.factor, (c.id, 'the record\'s factor was written')
        if c.f16_plant:
            assert float(o.rec[1]) > 0.0, (c.id, 'the saturated twin was not reported')
        else:
            assert float(o.rec[1]) == 0.0 and not torch.signbit(o.rec[1]), (c.id, 'overflow reported', float(o.rec[1]))
    return n


# ------------------------------------------------------------------------------------------------------------------ non-finite
NF_ACTS = (ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID)
NF_OTHER = (ACT_SILU, ACT_ELU, ACT_GELU, ACT_SELU, ACT_SOFTPLUS)      # form z * 0 at +-inf somewhere: only their NaN cases are compared
NF_ROWS_16 = [(5, (130, 128, 64)), (2, (32700, 512, 64)), (2, (65536, 256, 64)), (6, (49000, 256, 64))]      # row-per-lane epilogue
NF_SLAB_16 = [(5, (130, 132, 64))]
NF_SLAB_32 = [(5, (130, 132, 32)), (5, (130, 128, 32)), (3, (49000, 256, 32))]      # (N = 128: the bit twin needs N % 32 == 0)
# mask_out_colsum: the column sums send the launch to the slab on the row-per-lane shapes too - the slab's ReLU with a bit twin
NF_VARIANTS = ('plain', 'record', 'mask_out', 'colsum', 'mask_out_colsum')


def nan_bits(sign):
    """A quiet f32 NaN built from its bit pattern, sign clear (0) or set (1)."""
    return torch.tensor([0x7FC00000 | (sign << 31)], dtype=torch.int64).to(torch.int32).view(torch.float32)[0]


@dataclass(frozen=True)
class NFCase:
    kid: int
    M: int
    N: int
    K: int
    store: str
    act: int
    epilogue: str             # 'rows' | 'slab': what the plain launch of the shape takes (mask_out without ReLU and colsum: the slab)
    out_f32: bool = False

    @property
    def id(self):
        return f'{self.epilogue}-{self.M}x{self.N}x{self.K}-{self.store}{"-out_f32" if self.out_f32 else ""}-{ACT_NAME[self.act]}'


def nf_cases():
    out = []
    for lst, stores, epi in ((NF_ROWS_16, ('bf16', 'f16'), 'rows'), (NF_SLAB_16, ('bf16', 'f16'), 'slab'),
                             (NF_SLAB_32, ('f32', 'x3', 'h3'), 'slab')):
        for kid, (M, N, K) in lst:
            if K == 32 and M == 49000:
                stores_ = ('f32',)                 # the issue names the shape once: one storage mode reaches the leaf
            else:
                stores_ = stores
            for store in stores_:
                for act in NF_ACTS + (NF_OTHER if M <= 130 else ()):      # (smooth activations take the slab on every shape)
                    out.append(NFCase(kid, M, N, K, store, act, epi))
    for act in NF_ACTS:
        out.append(NFCase(5, 130, 132, 64, 'bf16', act, 'slab', out_f32=True))
    return out


def nf_shapes():
    out = [(M, N, K, code, kid) for kid, (M, N, K) in NF_ROWS_16 + NF_SLAB_16 for code in (BF16, F16)]
    return out + [(M, N, K, code, kid) for kid, (M, N, K) in NF_SLAB_32 for code in (F32, F32X3, F32H3)]


def nf_build(c):
    """Finite operands (ref_gemm's builder, z of a few units) and their planted twins: A with +NaN in a middle row and -NaN in row
    M - 1 (h3: a further row with one operand 2^ea times beyond half's range), bias with +NaN, -NaN, +inf, -inf in the first, two
    middle and the last valid column (which value sits where rotates with the activation).  expect: per element, what torch's
    activation gives for the f32 z - only its NON-FINITE structure is used, so the matrix product is not needed: a NaN row or
    column is NaN whatever the rest holds, an infinite column is act(+-inf)."""
    exps = (12, 11) if c.store == 'h3' else None
    cc = Case(c.kid, c.M, c.N, c.K, c.store, ACT_SILU, 'nf', out_f32=c.out_f32, exps=exps)
    A, B, bias, P, bound, n = _operands(c.M, c.N, c.K, 1.0, 0)
    b = SimpleNamespace()
    b.case, b.A, b.B, b.bias, b.n = cc, A, B, bias, n
    b.aux, b.aux_mode, b.aux_split, b.aux_delta = None, AUX_NONE, 0, 0
    b.A_nf, b.bias_nf = A.clone(), bias.clone()
    rows = {c.M // 2: nan_bits(0), c.M - 1: nan_bits(1)}
    for r, v in rows.items():
        b.A_nf[r, (3 * r) % c.K] = v
    b.nan_rows = sorted(rows)
    if c.store == 'h3':
        b.A_nf[c.M // 3, 1] = 2.0 ** (17 - exps[0])         # 2^17 after the scale: beyond 65504 ("turns the output into NaN")
        b.nan_rows.append(c.M // 3)
    vals = [nan_bits(0), nan_bits(1), torch.tensor(math.inf), torch.tensor(-math.inf)]
    cols = [0, c.N // 2 - 1, c.N // 2, c.N - 1]
    b.cols = {}
    for i, col in enumerate(cols):
        v = vals[(i + c.act) % 4]
        b.bias_nf[col] = v
        b.cols[col] = float(v)
    assert bool(torch.signbit(b.bias_nf[torch.isnan(b.bias_nf)]).any()) and not bool(torch.signbit(b.bias_nf[torch.isnan(b.bias_nf)]).all())
    # z's non-finite structure (finite entries: 0) and what torch stores for it
    b.z = z = torch.zeros(c.M, c.N)
    for col, v in b.cols.items():
        z[:, col] = v
    z[b.nan_rows] = math.nan
    b.affected = torch.zeros(c.M, c.N, dtype=torch.bool)
    b.affected[b.nan_rows] = True
    b.affected[:, cols] = True
    b.expect = ACT_FN[c.act](z)
    if c.act in NF_OTHER:                           # compare only their NaN cases; what they store at +-inf is recorded
        b.compare = b.affected & torch.isnan(z)
    else:
        b.compare = b.affected
    return b


def nf_check_stored(got, b, c, name, dtype):
    """The affected elements of a planted launch's stored values (C, or the z twin with act = NONE semantics) against torch."""
    exp = b.expect
    g, e = got.float()[b.compare], exp[b.compare]
    nan = torch.isnan(e)
    seen = {}
    if dtype == torch.float16:
        # the shared saturating conversion stores a NaN as NaN or +-65504 (from_f32<f16_t>: -65504) and as nothing else; inf -> 65504
        ok = torch.isnan(g[nan]) | (g[nan].abs() == F16_MAX)
        assert bool(ok.all()), (name, 'f16: a NaN element stored as', g[nan][~ok][:4].tolist(), int((~ok).sum()), 'of', int(nan.sum()))
        seen['f16 NaN stored as'] = sorted({('nan' if v != v else v) for v in g[nan].tolist()}, key=str)
        e = e.clamp(-F16_MAX, F16_MAX)
    else:
        assert bool(torch.isnan(g[nan]).all()), (name, 'a NaN element stored as', g[nan][~torch.isnan(g[nan])][:4].tolist(),
                                                 int((~torch.isnan(g[nan])).sum()), 'of', int(nan.sum()))
    assert torch.equal(g[~nan], e[~nan].to(dtype).float()), (name, 'infinite columns', g[~nan][g[~nan] != e[~nan].to(dtype).float()][:4].tolist())
    return seen


def nf_run(be, c, dev='cpu', record_seen=None, colsum_report=None):
    """The launches of a non-finite case (NF_VARIANTS: plain, with a record, with mask_out, with colsum, with both), each once
    without and once with the plants.  The bit twin of NONE / RELU / TANH needs N % 32 == 0: the shapes with N = 132 run it for the
    smooth activations' z twin only, (130, 128, K) carries it for the others.  Returns the number of elements compared."""
    b = nf_build(c)
    cc = b.case
    dt = cc.out_dtype
    n = 0
    for variant in NF_VARIANTS:
        twin, sums = variant.startswith('mask_out'), variant.endswith('colsum')
        if twin and c.act < ACT_SILU and c.N % 32 != 0:
            continue
        kw = dict(act=c.act, twin=twin, record=1.0 if variant == 'record' else 0.0, colsum_n=c.N - 4 if sums else 0)
        name = (c.id, variant)
        clean = launch(be, b, dev, **kw)
        dirty = launch(be, b, dev, A=b.A_nf, bias=b.bias_nf, **kw)
        assert bool(torch.isfinite(clean.C.float()).all()), (name, 'the launch without plants stored a non-finite value')
        # everything the plants do not reach: bitwise what the same launch gives without them
        keep = ~b.affected
        assert torch.equal(dirty.C[keep], clean.C[keep]), (name, 'unaffected elements changed', int((dirty.C[keep] != clean.C[keep]).sum()))
        seen = nf_check_stored(dirty.C, b, c, name, dt)
        if record_seen is not None:
            if c.act in NF_OTHER:
                inf = b.affected & ~b.compare
                seen['at +-inf stores'] = sorted({('nan' if v != v else v) for v in dirty.C.float()[inf].tolist()}, key=str)
            record_seen.setdefault(c.id, {}).update({f'{variant}: {k}': v for k, v in seen.items()})
        n += int(b.compare.sum())
        if variant == 'record':
            assert float(clean.rec[0]) == 1.0 and float(clean.rec[1]) == 0.0, (name, 'overflow reported without plants', clean.rec.tolist())
            assert float(dirty.rec[0]) == 1.0, (name, 'the record\'s factor was written')
            assert float(dirty.rec[1]) > 0.0, (name, 'stored NaN / inf / saturated values were not reported')
        if twin:
            if c.act >= ACT_SILU:                   # the z twin: the storage conversion of z itself
                st = R.STORE_DTYPE[c.store]
                assert torch.equal(dirty.twin[keep], clean.twin[keep]), (name, 'twin: unaffected elements changed')
                zb = SimpleNamespace(expect=b.z, compare=b.affected)
                nf_check_stored(dirty.twin, zb, c, name + ('twin',), st)
            else:
                bits = R.unpack_bits(dirty.twin, c.N)
                want = dirty.C.float() > 0
                assert torch.equal(bits, want), (name, 'mask_out bit != (stored C > 0)', int((bits != want).sum()),
                                                 'first (m, n)', (bits != want).nonzero()[0].tolist())
            n += c.M * c.N
        if sums:
            st = dirty.C.float()[:, :c.N - 4]
            nan_col = torch.isnan(st).any(0)
            assert bool(nan_col.all()) or dt == torch.float16      # (a NaN row reaches every column; f16 may store it as +-65504)
            assert bool(torch.isnan(dirty.colsum[nan_col]).all()), (name, 'colsum finite over a column that holds a NaN')
            fin = torch.isfinite(st).all(0)
            if bool(fin.any()):
                check_colsum(dirty.colsum[fin], dirty.C[:, :c.N - 4][:, fin], int(fin.sum()), name, c.kid)
            key = ('colsum', str(dt).replace('torch.', ''), f'k{c.kid}')
            check_colsum(clean.colsum, clean.C, c.N - 4, name, c.kid, colsum_report, key)
            n += c.N - 4
    return n
