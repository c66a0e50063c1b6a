"""Why the A operand's half split of the ASE_F32H3 kernels may be two fused instructions per element (csrc/gemm_nt_kernels.h,
split_f16_pair): hi = half(sa x) and lo = half(sa x - hi), each ONE rounding of an exactly formed value (v_fma_mix{lo,hi}_f16),
equal the earlier sequence's half(f32(sa x)) and half(f32(f32(sa x) - f32(hi))) bit for bit.

  sa is a power of two >= 1, so sa x is exact in f32 (or overflows to inf in both forms);
  sa x - hi is a multiple of the f32 ulp of sa x and at most half an ulp of hi in size, so it is exact in f32 as well;
  hence the single rounding to half of the exact value is the rounding to half of the f32 value.

One input class is outside that argument and is asserted on its own: a finite x whose sa x exceeds f32's range (|x| > 2^128 / sa).
hi is inf in both forms; lo is NaN in the f32 sequence (inf - inf) and the opposite infinity in the fused one (a finite value minus
inf).  Neither reaches an output: the three products of such an element sum to NaN in both forms (inf - inf, or inf times a zero).

f64 is the exact arithmetic here (a product with a power of two and a difference of two values this close are exact in it), and
numpy converts f64 to half with one rounding.  The same inputs run through the kernels in tests/test_gpu_h3_loop.py."""
import numpy as np
import pytest
import torch

from tests.emu_backend import half_split

EXPS = (6, 11, 12)                      # sa = 2^e: the value path's operand exponents
F32 = np.float32


def _around(v):
    """v and its two f32 neighbours."""
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


def edge_values(e):
    """(finite, overflowing): f32 edge inputs of the split at scale 2^e, both signs.  `finite` split into finite halves;
    `overflowing` have |sa x| >= 65520 (hi = inf), or are inf / NaN themselves."""
    sa = 2.0 ** e
    pos = [0.0, 1e-45, 1.1754942e-38, 2.0 ** -126]                      # zero, the smallest and largest f32 subnormal, the smallest normal
    for j in (-24, -14, -2, 0, 10, 15):                                 # half's round-to-nearest-even ties, scaled: sa x = 2^j (1 + t 2^-11)
        for t in (1, 2, 3):
            pos += _around(2.0 ** j * (1.0 + t * 2.0 ** -11) / sa)
    pos += _around(2.0 ** -25 / sa)                                      # the tie between 0 and half's smallest subnormal
    for thr in (2.0 ** -24, 2.0 ** -14, 2.0 ** -2, 65504.0):            # sa x straddling half's subnormal / normal / lo-normal / finite limits
        pos += _around(thr / sa)
    big = _around(65520.0 / sa)                                          # 65520 = the tie between 65504 and "2^16": rounds to inf
    pos.append(big[0])
    over = [big[1], big[2], F32(70000.0 / sa), F32(3.0e38), F32(np.inf)]
    fin = np.array(pos, dtype=F32)
    ovf = np.array(over, dtype=F32)
    fin, ovf = np.concatenate([fin, -fin]), np.concatenate([ovf, -ovf, np.array([np.nan], dtype=F32)])
    assert np.all(np.abs(fin.astype(np.float64) * sa) < 65520.0) and not np.any(np.abs(ovf.astype(np.float64) * sa) < 65520.0)
    return fin, ovf


def random_values(n, seed):
    """n f32 values, log-uniform over [2^-30, 2^6], both signs."""
    g = np.random.default_rng(seed)
    return (np.exp2(g.uniform(-30.0, 6.0, n)) * g.choice([-1.0, 1.0], n)).astype(F32)


def split_f32_steps(x, e):
    """The earlier instruction sequence: every step rounded to f32, then to half."""
    with np.errstate(over='ignore', invalid='ignore'):
        sx = x * F32(2.0 ** e)
        hi = sx.astype(np.float16)
        lo = (sx - hi.astype(F32)).astype(np.float16)
    return hi, lo


def split_exact(x, e):
    """The fused form: each half is one rounding of the exact value."""
    with np.errstate(over='ignore', invalid='ignore'):
        sx = x.astype(np.float64) * 2.0 ** e
        hi = sx.astype(np.float16)
        lo = (sx - hi.astype(np.float64)).astype(np.float16)
    return hi, lo


def beyond_f32(x, e):
    """Finite inputs whose scaled value no longer fits f32."""
    return np.isfinite(x) & (np.abs(x.astype(np.float64)) * 2.0 ** e > float(np.finfo(F32).max))


def same_halves(a, b):
    """Bitwise equal, NaNs compared by class (a NaN's payload is not part of the contract)."""
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint16)[~nan], b.view(np.uint16)[~nan]))


@pytest.fixture(scope='module')
def randoms():
    x = random_values(1 << 20, 20250)
    assert x.size >= 10 ** 6 and float(np.abs(x).min()) < 2.0 ** -29 and float(np.abs(x).max()) > 2.0 ** 5
    return x


@pytest.mark.parametrize('e', EXPS)
def test_fused_split_equals_the_f32_sequence(randoms, e):
    fin, ovf = edge_values(e)
    x = np.concatenate([fin, ovf, randoms])
    hi_x, lo_x = split_exact(x, e)
    hi_s, lo_s = split_f32_steps(x, e)
    # the premises, on every input: sa x is exact in f32, and so is sa x - hi
    with np.errstate(over='ignore', invalid='ignore'):
        sx32, sx64 = x * F32(2.0 ** e), x.astype(np.float64) * 2.0 ** e
        ok = np.isfinite(sx32)
        assert np.array_equal(sx32[ok].astype(np.float64), sx64[ok]) and bool(np.all(np.abs(sx64[~ok & ~np.isnan(x)]) > 3.4e38))
        d32, d64 = sx32 - hi_s.astype(F32), sx64 - hi_x.astype(np.float64)
        okd = np.isfinite(d64)
        assert np.array_equal(d32[okd].astype(np.float64), d64[okd])
    far = beyond_f32(x, e)
    assert same_halves(hi_x, hi_s)
    assert same_halves(lo_x[~far], lo_s[~far])
    assert far.sum() == 2 and np.all(np.isinf(hi_x[far])) and np.all(np.isnan(lo_s[far])) and np.array_equal(lo_x[far], -hi_x[far])
    # the edge list does what it is there for
    n = fin.size
    assert np.all(np.isfinite(hi_x[:n])) and np.all(np.isfinite(lo_x[:n])) and not np.any(np.isfinite(hi_x[n:n + ovf.size]))
    assert np.any((lo_x[:n] != 0) & (np.abs(lo_x[:n].astype(np.float64)) < 2.0 ** -14))           # a subnormal lo
    assert np.any((hi_x[:n] != 0) & (np.abs(hi_x[:n].astype(np.float64)) < 2.0 ** -14))           # a subnormal hi
    assert np.any(np.abs(hi_x[:n].astype(np.float64)) == 65504.0)


@pytest.mark.parametrize('e', EXPS)
def test_both_agree_with_the_emulator(randoms, e):
    fin, ovf = edge_values(e)
    x = np.concatenate([fin, ovf, randoms])
    hi_e, lo_e = half_split(torch.from_numpy(x), e, saturate=False)
    keep = ~beyond_f32(x, e)                                                     # (lo of those: see the module's docstring)
    for name, got, want in zip(('hi', 'lo'), split_exact(x, e), (hi_e, lo_e)):
        want = want.numpy().astype(np.float16)                                   # (f64 carriers of half values: exact)
        assert same_halves(got, want) if name == 'hi' else same_halves(got[keep], want[keep])
