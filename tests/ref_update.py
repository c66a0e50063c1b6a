"""Plain CPU reference of the running-statistics, gather and optimizer kernels (csrc/rms.hip, csrc/optim.hip) - TEST
INFRASTRUCTURE ONLY.  Every operation is the reference's own expression (oracle/restated.py: rl_games RunningMeanStd, torch's
_single_tensor_adam, clip_grad_norm_; torch's own .to(dtype)) with a ``dtype`` argument, run in f64 and in f32; e_ref is
|f32 run - f64 run| on the same inputs.  tests/emu_backend.py restates the kernels by the same hand as the kernels; this file
shares nothing with it (the row map is tests/ref_rollout.py::row_map).  The case builders and one check_* body per operation
live here: tests/test_gpu_update.py runs them over HipBackend, tests/test_update_ref.py over the emulator on the CPU.

Every output lives inside a larger allocation with a row pitch wider than its payload, NaN (integers: SENT_I) everywhere else;
sources carry NaN in their pitch columns and in every row the row map does not reach; all sentinels are checked after every
launch and no element is left out of a comparison.

The bounds
  rms_moments / rms_moments_multi ('sums +=', every slot starts at ACC0 = 0.5).  include/ase_hip.h fixes the term exactly:
      (double)(x - f32(mean)), the subtraction in f32; its square is exact in f64 (24 + 24 bits).  Only the order of the f64
      additions is free, so |got - (ACC0 + sum)| <= n 2^-53 sum |term| + 2^-53 |ACC0 + sum| (n - 1 roundings of partial sums
      that never exceed sum |term|, and the roundings of the additions into the slot, at most the slot's magnitude each; the
      second kind is only more than one when M > 64, where n sum |term| dwarfs it).  No e_ref enters.
  rms_finalize.  State (f64 mean, var): per tensor 2 e_ref + 2^-24 max |ref| - the kernel rounds the batch mean and variance
      to f32 on purpose (as torch's x.mean(0) / x.var(0) on f32 data are f32), half an f32 ulp of the largest entry.
      mean_out / std_out: `within` of tests/ref_heads.py, 2 e_ref + 2^-23 max |ref|.  The count: exact.
  rms_normalize* / rms_unnormalize: `within`, + half a storage ulp.  mean and std are the f32 tensors the kernel is given
      (restated.rms_normalize with var = std^2 and eps = 0: sqrt(fl(s^2)) == s in binary floating point).  +-inf -> +-5, beyond
      the clamp -> +-5, (x - mean) / std == +-5 -> +-5 and NaN -> NaN hold exactly (torch.clamp keeps NaN).
  adam, axpy and apply_multi's W, m, v, bias and exported gradient: per element |got - f64|_i <= 2 e_ref,i + c 2^-24 S_i with S_i the
      sum of the magnitudes of the terms of element i's expression in f64 and c the f32 roundings counted from adam_elem
      (sqrtf and / count twice: within 1 ulp, not correctly rounded):
        m = m0 + f32(1 - b1) (g - m0): the scalar, the subtraction, the product / addition (contracted or not)      c = 3
        v = v0 b2 + f32(1 - b2) g g: two scalars, two products, (one addition)                                       c = 4
        w = w0 - f32(lr / bc1) (m / (sqrtf(v) / f32(sqrt(bc2)) + eps)): sqrtf 2, / 2, + eps 1, / 2, the product / subtraction 1;
            the errors of m and v themselves reach w through the reference's own e_ref                               c = 8
        exported gradient g + c w: the product and the addition                                                      c = 2
      S_m = |m0| + (1 - b1) |g - m0|, S_v = |v_new|, S_w = |w0| + |update|, S_g = |g| + |c w|.
  apply_multi's shadows and bias copy: bitwise the conversion of the W / bias the kernel itself stored, concat columns at
      k + gap past split_src.  Sum-of-squares slots: the f64 sum of the pre-update w^2 (each exact in f64) by the bound of the moments.
  begin_step: the step exact; bias_corr within 8 2^-53 absolute of Python's 1 - beta ** step (pow is within a few ulp of a
      number below 1); zeroed ranges exactly 0, the word after each intact; rng_bump[1] + 1, rng_bump[0] untouched.
  clip_scale: `within` against restated.clip_grad_norm's coefficient in f64; a norm under the bound leaves the buffer bitwise.
  gather_rows / gather_multi / convert_multi: bitwise torch's own .to(dtype) - IEEE half after a clamp to +-65504, the header's
      'saturating'.  What the saturating conversion does to a NaN is recorded here: F16_OF_NAN."""
import math
import struct

import torch

from oracle import restated as R
from tests.ref_heads import F32, F64, NAN, STATS, _name, _nanbuf, _note, f32, half_ulp, within   # noqa: F401
from tests.ref_rollout import row_map

BF16, F16 = torch.bfloat16, torch.float16
STORAGES = (F32, BF16, F16)
CODE = {F32: 0, BF16: 1, F16: 3}          # ASE_F32 / ASE_BF16 / ASE_F16 (compared with ase_amd.lib by tests/test_update_ref.py)
ACC0 = 0.5
SENT_I = 0x5A5A5A5A5A5A5A5A
# from_f32<f16_t> clamps with the hardware's median-of-three, which returns the MINIMUM of its operands when one is a NaN:
# a NaN converted into IEEE half storage by the saturating conversion is stored as -65504 (include/ase_hip.h, 'saturating')
F16_OF_NAN = -65504.0
COUNTS = {'cases': 0, 'elements': 0, 'sentinels': 0}
OPS = ('rms_moments', 'rms_finalize', 'rms_normalize', 'rms_unnormalize', 'adam', 'axpy', 'clip_scale', 'apply_multi')


def nanbuf(shape, dev, dtype=F32):
    return _nanbuf(shape if isinstance(shape, tuple) else (shape,), dev, dtype)


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def _sent(t, what):
    t = t.detach().cpu()
    assert bool(torch.isnan(t.float()).all()), (what, 'sentinel overwritten')
    COUNTS['sentinels'] += t.numel()


def padded(x, pitch, dev, off=0, extra=1, shift=0, fill=NAN):
    """x [r, c] at column `off` of a NaN allocation [r + extra, pitch] that starts `shift` elements into its buffer."""
    r, c = x.shape
    assert pitch >= off + c
    flat = torch.full(((r + extra) * pitch + shift,), fill, dtype=x.dtype)
    flat[shift:].view(r + extra, pitch)[:r, off:off + c] = x
    return flat.to(dev)[shift:].view(r + extra, pitch)


def outside(buf, rows, off, cols, what):
    """Every element of buf outside [0, rows) x [off, off + cols) is still the NaN it was allocated with."""
    t = buf.detach().float().cpu()
    m = torch.ones_like(t, dtype=torch.bool)
    m[:rows, off:off + cols] = False
    assert bool(torch.isnan(t[m]).all()), (what, 'sentinel overwritten')
    COUNTS['sentinels'] += int(m.sum())


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def same(got, want, what):
    """torch.equal that tells -0.0 from 0.0 and takes NaN for NaN (whatever its payload)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    n = torch.isnan(want.float()) if want.is_floating_point() else torch.zeros_like(want, dtype=torch.bool)
    if want.is_floating_point():
        assert torch.equal(torch.isnan(got.float()), n), (what, 'NaN entries differ', int(torch.isnan(got.float()).sum()), int(n.sum()))
    bad = (bits(got) != bits(want)) & ~n
    assert not bad.any(), (what, 'elements differ', int(bad.sum()), bad.nonzero()[:4].tolist())
    COUNTS['elements'] += want.numel()


def convert(x, storage):
    """torch's own conversion; IEEE half saturates (a clamp to +-65504 first) and stores F16_OF_NAN for a NaN."""
    if storage == F16:
        x = torch.where(torch.isnan(x), torch.full_like(x, F16_OF_NAN), x.clamp(-65504.0, 65504.0))
    return x.to(storage)


def sum_bound(got, terms, name, key=None, start=ACC0):
    """A slot that started at `start` and received the f64 sum of `terms` [n, cols] (exact f64 values) in some order."""
    t = terms.detach().double()
    n = t.shape[0]
    want = t.sum(0) + start
    tol = n * 2.0 ** -53 * t.abs().sum(0) + 2.0 ** -53 * want.abs()
    got = got.detach().double().cpu().reshape(want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, 'NaN slots differ')
    err = (got - want).abs()
    print(f'{name}: max |sum - f64| = {float(err.max()):.3g}, allowance {float(tol.max()):.3g} (n = {n})')
    assert bool((err <= tol).all()), (name, float(err.max()), float(tol.max()), (err > tol).nonzero()[:4].tolist())
    COUNTS['elements'] += want.numel()
    if key:
        _note(key + ('f64',), float(err.max()), 0.0, want.numel())


def state_within(got, r64, r32, name, key=None):
    """Per tensor: max |got - f64| <= 2 e_ref + 2^-24 max |ref|."""
    got, r64, r32 = got.detach().double().cpu(), r64.double(), r32.double()
    e_ref = float((r32 - r64).abs().max())
    tol = 2 * e_ref + 2.0 ** -24 * float(r64.abs().max())
    err = float((got - r64).abs().max())
    print(f'{name}: max |got - f64| = {err:.3g}, e_ref = {e_ref:.3g}, allowance {tol:.3g}')
    assert err <= tol, (name, err, tol)
    COUNTS['elements'] += r64.numel()
    if key:
        _note(key + ('f64',), err, e_ref, r64.numel())


def elem_within(got, r64, r32, S, c, name, key=None):
    """Per element: |got - f64|_i <= 2 e_ref,i + c 2^-24 S_i.  Non-finite entries are equal as such."""
    got, r64, r32, S = got.detach().double().cpu().reshape(r64.shape), r64.double(), r32.double(), S.double()
    fin = torch.isfinite(r64)
    assert torch.equal(torch.isnan(got), torch.isnan(r64)), (name, 'NaN entries differ')
    assert torch.equal(got[~fin & ~torch.isnan(r64)], r64[~fin & ~torch.isnan(r64)]), (name, 'infinite entries differ')
    e = (r32 - r64).abs()
    tol = 2 * e + c * 2.0 ** -24 * S
    err = (got - r64).abs()
    bad = fin & ~(err <= tol)
    r = (err[fin] / tol[fin].clamp_min(1e-300))
    print(f'{name}: max |got - f64| = {float(err[fin].max()):.3g}, max e_ref = {float(e[fin].max()):.3g}, worst err / allowance '
          f'{float(r.max()):.3g} (c = {c})')
    assert not bad.any(), (name, 'elements over the bound', int(bad.sum()), bad.nonzero()[:4].tolist(), float(r.max()))
    COUNTS['elements'] += r64.numel()
    if key:
        _note(key + ('f32',), float(err[fin].max()), float(e[fin].max()), int(fin.sum()))


# ------------------------------------------------------------------------------------------------ running statistics
RMS_M = (2, 63, 64, 65, 129, 300)
RMS_D = (1, 3, 4, 63, 64, 65, 253, 260)
FAMILIES = {'plain': (0.5, 2.0, 1.0, 0.0), 'offset': (1e3, 1e-2, 1.0, 0.0), 'warm': (1e3, 1e-2, 1e6, 1e3), 'const': (0.5, 2.0, 1.0, 0.0)}
RMS_PATHS = ('wide', 'idx', 'off1', 'oddld', 'dup', 'idx_remap', 'remap', 'remap_scalar')


def moments_wide(src, D, idx):
    """The entry's condition for the 16-byte kernel (csrc/rms.hip ase_hip_rms_moments)."""
    return idx is None and D % 4 == 0 and src.stride(0) % 4 == 0 and src.data_ptr() % 16 == 0


def finalize_threads(D):
    return 1024 if D > 256 else 256


def rms_stream(M, D, path, family, seed):
    """One source: payload x [rows, D] (NaN in every row the map does not reach), idx, remap, pitch, shift."""
    g = torch.Generator().manual_seed(seed)
    off, spread, _, _ = FAMILIES[family]
    remap = (0, 0)
    rows = M
    if 'remap' in path:
        H = 3 if M > 2 else 2
        remap = (H, (M + H - 1) // H + 1)
        rows = remap[0] * remap[1]
    if path in ('idx', 'dup', 'idx_remap'):
        rows = max(rows, M + 7)
    idx = None
    if path in ('idx', 'idx_remap'):
        idx = torch.randperm(rows, generator=g)[:M].to(torch.int32)
    elif path == 'dup':
        idx = torch.randint(0, rows, (M,), generator=g).to(torch.int32)
        idx[M - 1] = idx[0]
    x = off + spread * torch.randn(rows, D, generator=g)
    if family == 'const':
        x[:, D // 2] = 0.75
    p = row_map(idx, remap, M)
    assert int(p.max()) < rows and int(p.min()) >= 0
    dead = torch.ones(rows, dtype=torch.bool)
    dead[p] = False
    x[dead] = NAN
    pitch = (D + 3) // 4 * 4 + 4
    if path in ('oddld', 'remap_scalar'):
        pitch = D + 1 if (D + 1) % 4 else D + 2
    return {'x': x, 'idx': idx, 'remap': remap, 'pitch': pitch, 'shift': 1 if path == 'off1' else 0, 'rows': x[p], 'path': path,
            'wide': path in ('wide', 'remap') and D % 4 == 0}


def rms_case(M, D, path='wide', family='plain', n_streams=1, seed=0):
    g = torch.Generator().manual_seed(31 * M + D + seed)
    _, spread, count, mean = FAMILIES[family]
    st = torch.empty(2 * D + 1, dtype=F64)
    st[:D] = mean + 1e-3 * torch.randn(D, generator=g, dtype=F64)           # (not an f32 number: the shift is f32(mean))
    st[D:2 * D] = 1.0 if count == 1.0 else spread ** 2
    st[2 * D] = count
    return {'name': f'M{M} D{D} {path} {family} x{n_streams}', 'M': M, 'D': D, 'family': family, 'state': st,
            'streams': [rms_stream(M, D, path, family, 1000 * s + 7 * M + D + seed) for s in range(n_streams)]}


def rms_terms(c, s):
    """The header's term of every gathered row: (double)(x - f32(mean)), the subtraction in f32."""
    D = c['D']
    return (c['streams'][s]['rows'] - c['state'][:D].float()).double()


def rms_update_ref(c, dtype, upto=None, rows=None):
    """restated.rms_update over the streams in order; returns the state after each merge."""
    D = c['D']
    s = {'mean': c['state'][:D].to(dtype), 'var': c['state'][D:2 * D].to(dtype), 'count': c['state'][2 * D].to(dtype)}
    out = []
    for st in c['streams'][:upto]:
        R.rms_update(s, (st['rows'] if rows is None else rows).to(dtype))
        out.append(R.rms_clone(s))
    return out


def _rms_src(st, dev):
    return padded(st['x'], st['pitch'], dev, shift=st['shift']), None if st['idx'] is None else st['idx'].to(dev)


def _sums(n, D, dev, start):
    buf = torch.full((n * 2 * D + 3,), NAN, dtype=F64)
    buf[:n * 2 * D] = start
    return buf.to(dev)


def run_moments(b, dev, c, start, multi):
    """-> the sums buffer [n 2 D + 3 sentinels] on the device after one launch per stream, or one launch for all."""
    M, D, n = c['M'], c['D'], len(c['streams'])
    state = torch.cat([c['state'], torch.full((1,), NAN, dtype=F64)]).to(dev)
    sums = _sums(n, D, dev, start)
    srcs = [_rms_src(st, dev) for st in c['streams']]
    for st, (src, idx) in zip(c['streams'], srcs):
        assert moments_wide(src, D, idx) == st['wide'], (c['name'], 'the case does not reach the kernel it is meant for')
    if multi:
        b.rms_moments_multi([(src, idx, st['remap']) for st, (src, idx) in zip(c['streams'], srcs)], D, M, state[:2 * D + 1],
                            [sums[s * 2 * D:(s + 1) * 2 * D] for s in range(n)])
    else:
        for s, (st, (src, idx)) in enumerate(zip(c['streams'], srcs)):
            b.rms_moments(src, D, idx, st['remap'], M, state[:2 * D + 1], sums[s * 2 * D:(s + 1) * 2 * D])
    _sync(dev)
    same(state, torch.cat([c['state'], torch.full((1,), NAN, dtype=F64)]), 'rms_moments leaves the state alone')
    _sent(sums[n * 2 * D:], 'sums')
    return sums


def check_moments(b, dev, c, who, multi=False):
    D, n = c['D'], len(c['streams'])
    got = run_moments(b, dev, c, ACC0, multi).cpu()[:n * 2 * D].view(n, 2 * D)
    tag = f'{who} rms_moments{"_multi" if multi else ""} {c["name"]}'
    for s in range(n):
        d = rms_terms(c, s)
        sum_bound(got[s, :D], d, f'{tag} s1[{s}]', ('rms_moments', 's1'))
        sum_bound(got[s, D:], d * d, f'{tag} s2[{s}]', ('rms_moments', 's2'))
    COUNTS['cases'] += 1
    return got


def check_finalize(b, dev, c, who, multi=False, sums=None, count=None, refs=None):
    """Moments from zero, then the merge of all streams in one rms_finalize: state, mean_out / std_out per stream, count."""
    M, D, n = c['M'], c['D'], len(c['streams'])
    sums = run_moments(b, dev, c, 0.0, multi) if sums is None else sums
    state = torch.cat([c['state'], torch.full((1,), NAN, dtype=F64)]).to(dev)
    mo, so = nanbuf((n + 1) * D, dev), nanbuf((n + 1) * D, dev)
    b.rms_finalize(state[:2 * D + 1], D, sums[:n * 2 * D], M if count is None else count, n, mo[:n * D], so[:n * D])
    _sync(dev)
    state, mo, so = state.cpu(), mo.cpu(), so.cpu()
    _sent(state[2 * D + 1:], 'state')
    _sent(mo[n * D:], 'mean_out')
    _sent(so[n * D:], 'std_out')
    r64, r32 = refs if refs is not None else (rms_update_ref(c, F64), rms_update_ref(c, F32))
    tag, key = f'{who} rms_finalize {c["name"]} [{finalize_threads(D)} threads]', ('rms_finalize',)
    state_within(state[:D], r64[-1]['mean'], r32[-1]['mean'], tag + ' mean', key + ('mean',))
    state_within(state[D:2 * D], r64[-1]['var'], r32[-1]['var'], tag + ' var', key + ('var',))
    assert float(state[2 * D]) == float(r64[-1]['count']), (tag, 'count', float(state[2 * D]), float(r64[-1]['count']))
    for s in range(n):
        within(mo[s * D:(s + 1) * D], r64[s]['mean'], r32[s]['mean'], f'{tag} mean_out[{s}]', key=key + ('mean_out',))
        within(so[s * D:(s + 1) * D], torch.sqrt(r64[s]['var'] + 1e-5), torch.sqrt(r32[s]['var'] + 1e-5), f'{tag} std_out[{s}]',
               key=key + ('std_out',))
    COUNTS['cases'] += 1
    COUNTS['elements'] += 2 * n * D + 1
    return state


def check_halves(b, dev, c, who):
    """The data-parallel use: two half batches accumulated into one `sums`, merged with count = the total."""
    M, D = c['M'], c['D']
    st = c['streams'][0]
    assert st['idx'] is None and st['remap'] == (0, 0) and M >= 4
    h = M // 2
    state = c['state'].to(dev)
    sums = _sums(1, D, dev, 0.0)
    src, _ = _rms_src(st, dev)
    b.rms_moments(src, D, None, (0, 0), h, state, sums[:2 * D])
    b.rms_moments(src[h:], D, None, (0, 0), M - h, state, sums[:2 * D])
    check_finalize(b, dev, c, who + ' two halves', sums=sums, count=M)


def check_eval(b, dev, c, who):
    """n_streams 0: the state bitwise unchanged, mean_out = f32(mean), std_out = sqrt(f32(var) + 1e-5)."""
    D = c['D']
    state = torch.cat([c['state'], torch.full((1,), NAN, dtype=F64)]).to(dev)
    mo, so = nanbuf(D + 1, dev), nanbuf(D + 1, dev)
    b.rms_finalize(state[:2 * D + 1], D, None, 0, 0, mo[:D], so[:D])
    _sync(dev)
    same(state, torch.cat([c['state'], torch.full((1,), NAN, dtype=F64)]), 'eval mode: the state')
    _sent(mo[D:], 'mean_out')
    _sent(so[D:], 'std_out')
    var = c['state'][D:2 * D]
    same(mo[:D], c['state'][:D].float(), 'eval mean_out')
    within(so[:D], torch.sqrt(var + 1e-5), torch.sqrt(var.float() + 1e-5), f'{who} rms_finalize eval {c["name"]} std_out',
           key=('rms_finalize', 'std_out eval'))
    COUNTS['cases'] += 1


def moments_plan():
    """(case, multi).  Every (M, D) on the aligned path; every path x family at four shapes; 1 / 3 / 4 streams."""
    out = [(rms_case(M, D), False) for M in RMS_M for D in RMS_D]
    for path in RMS_PATHS:
        for fam in FAMILIES:
            for M, D in ((65, 260), (129, 64), (300, 253), (2, 4)):
                out.append((rms_case(M, D, path, fam, seed=3), False))
    for n in (1, 3, 4):
        for M, D, path in ((129, 260, 'idx_remap'), (65, 65, 'dup'), (64, 4, 'remap'), (2, 1, 'idx')):
            out.append((rms_case(M, D, path, 'offset' if n == 3 else 'plain', n, seed=5), True))
    return out


def finalize_plan():
    out = [(rms_case(M, D, 'wide', fam, seed=11), False) for fam in FAMILIES for M, D in ((2, 3), (65, 260), (300, 253), (129, 64))]
    out += [(rms_case(M, D, 'idx_remap', fam, 3, seed=13), True) for fam in FAMILIES for M, D in ((2, 4), (129, 260), (300, 65))]
    out += [(rms_case(65, 1400, 'idx', 'warm', 2, seed=17), True), (rms_case(63, 1, 'wide', 'offset', 1, seed=19), False)]
    return out


# ------------------------------------------------------------------------------------------------ normalise / unnormalise
SPECIALS = (NAN, float('inf'), float('-inf'), 100.0, -100.0, 2.5, -2.5)       # +-2.5: (x - 0) / 0.5 == +-5 exactly
NORM_D = (1, 3, 4, 253, 257, 260)
NORM_M = (1, 3, 4, 5, 300)
NORM_KERNELS = ('scalar', 'wide', 'multi', 'twin')


def norm_case(M, D, kernel, n_out=1, mapped=False, seed=0):
    """x with the specials in the first row, the last row and the last column; mean 0 / std 0.5 in every third column and the
    last one (the exact +-5 entries live there), std = sqrt(1e-5) (a constant column's) in column 1."""
    g = torch.Generator().manual_seed(97 * M + D + seed)
    remap, rows, idx = (0, 0), M, None
    if mapped:
        remap = (2, (M + 1) // 2 + 1)
        rows = remap[0] * remap[1] + 3
        idx = torch.randperm(remap[0] * remap[1], generator=g)[:M].to(torch.int32)
    mean, std = torch.randn(D, generator=g), torch.exp(0.5 * torch.randn(D, generator=g))
    edge = torch.zeros(D, dtype=torch.bool)
    edge[::3] = True
    edge[D - 1] = True
    mean[edge], std[edge] = 0.0, 0.5
    if D > 2:
        std[1] = f32(math.sqrt(1e-5))
    y = torch.randn(M, D, generator=g) * 2.5                   # a good part of it beyond the clamp
    x = y * std + mean
    sp = torch.zeros(M, D, dtype=torch.bool)
    k = 0
    for r in {0, M - 1}:
        for j in range(D):
            v = SPECIALS[(j + r) % 7]
            x[r, j] = v if (edge[j] or abs(v) != 2.5) else 100.0 * v
            sp[r, j] = True
    for r in range(M):
        x[r, D - 1] = SPECIALS[(r + k) % 7]
        sp[r, D - 1] = True
    p = row_map(idx, remap, M)
    full = torch.full((rows, D), NAN)
    full[p] = x
    wide = kernel != 'scalar'
    assert not wide or D % 4 == 0
    pitch = (D + 3) // 4 * 4 + 4
    if kernel == 'scalar' and D % 4 == 0:
        pitch += 1                                              # an odd source pitch takes a 4-column width off the 16-byte path
    outs = [((D + 3) // 4 * 4 + 4 * (o + 1), 4 * o) for o in range(n_out)]      # (pitch, column offset) per output
    return {'name': f'M{M} D{D} {kernel} outs{n_out} mapped={int(mapped)}', 'M': M, 'D': D, 'kernel': kernel, 'x': x, 'full': full,
            'idx': idx, 'remap': remap, 'mean': mean, 'std': std, 'pitch': pitch, 'outs': outs, 'special': sp, 'wide': wide}


def normalize_ref(c, dtype):
    return R.rms_normalize({'mean': c['mean'].double(), 'var': c['std'].double() ** 2}, c['x'].to(dtype), eps=0.0)


def normalize_wide(src, D, mean, std, outs):
    """The entry's condition for rms_normalize4_kernel (csrc/rms.hip ase_hip_rms_normalize)."""
    ok = all(o is None or (o.stride(0) % 4 == 0 and o.data_ptr() % (4 * o.element_size()) == 0) for o in outs)
    return D % 4 == 0 and src.stride(0) % 4 == 0 and src.data_ptr() % 16 == 0 and mean.data_ptr() % 16 == 0 and std.data_ptr() % 16 == 0 and ok


def run_normalize(b, dev, c, storage, kernel=None):
    """-> [(buffer, column offset)] per output, and the twin's buffer (or None)."""
    M, D, kernel = c['M'], c['D'], kernel or c['kernel']
    src = padded(c['full'], c['pitch'], dev)
    idx = None if c['idx'] is None else c['idx'].to(dev)
    mean, std = c['mean'].to(dev), c['std'].to(dev)
    bufs = [nanbuf((M + 1, p), dev, storage) for p, _ in c['outs']]
    wins = [bf[:, o:] for bf, (_, o) in zip(bufs, c['outs'])]
    twin = None
    if kernel in ('scalar', 'wide'):
        assert normalize_wide(src, D, mean, std, wins) == (kernel == 'wide'), (c['name'], 'not the kernel the case is meant for')
        b.rms_normalize(src, D, idx, c['remap'], M, mean, std, wins)
    else:
        # one stream per output; every stream has a source, a row map and statistics of its own (here: the same values)
        streams = [(src, idx, c['remap'])] * len(wins)
        if kernel == 'multi':
            b.rms_normalize_multi(streams, D, M, [mean] * len(wins), [std] * len(wins), wins)
        else:
            twin = nanbuf((M + 1, D + 4), dev)
            b.rms_normalize_multi_twin(streams, D, M, [mean] * len(wins), [std] * len(wins), wins, [twin] + [None] * (len(wins) - 1))
    _sync(dev)
    return [(bf.cpu(), o) for bf, (_, o) in zip(bufs, c['outs'])], None if twin is None else twin.cpu()


def check_normalize(b, dev, c, storage, who, ref=None):
    M, D = c['M'], c['D']
    r64, r32 = ref if ref is not None else (normalize_ref(c, F64), normalize_ref(c, F32))
    outs, twin = run_normalize(b, dev, c, storage)
    tag, sp = f'{who} rms_normalize {c["name"]}', c['special']
    for i, (bf, o) in enumerate(outs):
        outside(bf, M, o, D, tag)
        got = bf[:M, o:o + D]
        within(got, r64, r32, f'{tag} out{i}', storage=storage, key=('rms_normalize', c['kernel']))
        same(got[sp].float(), r64[sp].float(), f'{tag} out{i}: the special elements hold exactly')      # NaN, +-5
        if i:
            same(got, outs[0][0][:M, outs[0][1]:outs[0][1] + D], f'{tag}: every output stores the same value')
    if twin is not None:
        outside(twin, M, 0, D, tag + ' twin')
        f = dict(c, outs=c['outs'][:1])
        ref32, _ = run_normalize(b, dev, f, F32, 'multi')
        same(twin[:M, :D], ref32[0][0][:M, ref32[0][1]:ref32[0][1] + D], tag + ': the twin is bitwise an f32-storage call')
    COUNTS['cases'] += 1
    COUNTS['elements'] += len(outs) * M * D


def normalize_plan():
    """Case keyword lists; storage types are the tests' parameter."""
    out = []
    for D in NORM_D:
        for M in NORM_M:
            for kernel in NORM_KERNELS:
                if kernel != 'scalar' and D % 4:
                    continue
                n_out = 1 + (M + D) % 3
                out.append(dict(M=M, D=D, kernel=kernel, n_out=n_out, mapped=(M + D) % 2 == 0))
    return out


UNNORM_N = (1, 255, 100003, 2048 * 256 + 1)


def unnorm_case(n, seed=0):
    g = torch.Generator().manual_seed(n + seed)
    x = torch.randn(n, generator=g) * 4
    sp = (NAN, float('inf'), float('-inf'), 100.0, -100.0, 5.0, -5.0)
    pos = [0] if n == 1 else list(range(min(7, n))) + [n - 1 - i for i in range(min(7, n - 7))]
    for k, i in enumerate(pos):
        x[i] = sp[k % 7]
    return {'n': n, 'x': x, 'pos': torch.tensor(pos), 'mean': 1.25 + 1e-9, 'var': 7.3}


def check_unnormalize(b, dev, c, who):
    n = c['n']
    x = torch.cat([c['x'], torch.full((1,), NAN)]).to(dev)
    y = nanbuf(n + 1, dev)
    state = torch.tensor([c['mean'], c['var'], 10.0, NAN], dtype=F64).to(dev)
    b.rms_unnormalize(state[:3], x[:n], y[:n])
    _sync(dev)
    y = y.cpu()
    _sent(y[n:], 'rms_unnormalize y')
    s = {'mean': torch.tensor(c['mean'], dtype=F64), 'var': torch.tensor(c['var'], dtype=F64)}
    r64, r32 = R.rms_unnormalize(s, c['x'].double()), R.rms_unnormalize(s, c['x'])
    within(y[:n], r64, r32, f'{who} rms_unnormalize n{n}', key=('rms_unnormalize', 'y'))
    pos = c['pos']
    assert torch.equal(torch.isnan(y[pos]), torch.isnan(r64[pos])) and int(torch.isnan(r64[pos]).sum()) >= 1
    hi = y[:n][c['x'] >= 5.0]                          # +inf, 100 and 5 itself: one value, and the same for the other side
    lo = y[:n][c['x'] <= -5.0]
    assert (hi.numel() == 0 or bool((hi == hi[0]).all())) and (lo.numel() == 0 or bool((lo == lo[0]).all())), 'beyond the clamp: one value'
    COUNTS['cases'] += 1
    COUNTS['elements'] += n


# ------------------------------------------------------------------------------------------------ gather / convert
GATHER_D = (1, 2, 3, 31, 33, 64, 65, 140)
GATHER_M = (1, 255, 257)
# RNE ties of both 16-bit types (to even, both ways), beyond half's range, a half subnormal, -0.0, +-inf, NaN
VALUES = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0, -70000.0, 2.0 ** -24 * 3, 2.0 ** -25,
          -0.0, float('inf'), float('-inf'), NAN, 65519.9, 65520.0)


def gather_width(D):
    """The lane-group width the entry chooses (csrc/rms.hip ase_hip_gather_rows)."""
    W = 64
    while W > 1 and W // 2 >= D:
        W //= 2
    return W


def gather_src(rows, D, g):
    x = torch.randn(rows, D, generator=g) * 3
    flat = x.view(-1)
    n = min(len(VALUES), flat.numel())
    flat[:n] = torch.tensor(VALUES[:n])
    if flat.numel() > 2 * len(VALUES):
        flat[-len(VALUES):] = torch.tensor(VALUES)
    return x


def check_gather_rows(b, dev, M, D, storage, who):
    g = torch.Generator().manual_seed(13 * M + D)
    remap = (3, (M + 2) // 3 + 1)
    rows = remap[0] * remap[1]
    idx = torch.randperm(rows, generator=g)[:M].to(torch.int32)
    x = gather_src(rows, D, g)
    src = padded(x, D + 3, dev)
    dst = nanbuf((M + 1, D + 5), dev, storage)
    b.gather_rows(src, D, idx.to(dev), remap, M, dst[:, 2:])
    _sync(dev)
    outside(dst, M, 2, D, f'{who} gather_rows')
    same(dst.cpu()[:M, 2:2 + D], convert(x[row_map(idx, remap, M)], storage), f'{who} gather_rows M{M} D{D} W{gather_width(D)} {_name(storage)}')
    COUNTS['cases'] += 1


def convert_vec(src, D, dst):
    """convert_multi_kernel's condition for 8 values per thread (csrc/rms.hip)."""
    return (dst.dtype != F32 and D % 8 == 0 and src.stride(0) % 4 == 0 and dst.stride(0) % 8 == 0 and src.data_ptr() % 16 == 0
            and dst.data_ptr() % 16 == 0)


def run_gather_multi(b, dev, fields, idx, remap, M, who):
    """fields: [(x [rows, D], storage, src pitch, dst pitch, src shift, dst shift)] in ONE launch.  -> per field whether the
    identity map's 8-wide path applies."""
    srcs, dsts, vec = [], [], []
    for x, st, ps, pd, ss, ds in fields:
        srcs.append(padded(x, ps, dev, shift=ss))
        flat = nanbuf(((M + 1) * pd + ds,), dev, st)
        dsts.append(flat[ds:].view(M + 1, pd))
    items = [(s, f[0].shape[1], d) for s, d, f in zip(srcs, dsts, fields)]
    desc = torch.tensor([[s.data_ptr(), s.stride(0), D, d.data_ptr(), d.stride(0), CODE[d.dtype]] for s, D, d in items], dtype=torch.int64).to(dev)
    b.gather_multi(desc, items, None if idx is None else idx.to(dev), remap, M)
    _sync(dev)
    p = row_map(idx, remap, M)
    for (x, st, *_), (s, D, d) in zip(fields, items):
        outside(d, M, 0, D, f'{who} gather_multi')
        same(d.cpu()[:M, :D], convert(x[p], st), f'{who} gather_multi M{M} D{D} {_name(st)}')
        vec.append(convert_vec(s, D, d))
    COUNTS['cases'] += 1
    return vec


def check_gather_multi(b, dev, M, who, rot=0):
    """Fields of widths 1, 31, 64, 253 with a different storage type per field, gathered through idx and remap."""
    g = torch.Generator().manual_seed(17 * M + rot)
    remap = (2, (M + 1) // 2 + 2)
    rows = remap[0] * remap[1]
    idx = torch.randperm(rows, generator=g)[:M].to(torch.int32)
    fields = [(gather_src(rows, D, g), STORAGES[(i + rot) % 3], D + 1 + i, D + 3 + i, 0, 0) for i, D in enumerate((1, 31, 64, 253))]
    run_gather_multi(b, dev, fields, idx, remap, M, who)


# (D, src pitch, dst pitch, src shift, dst shift) of the identity map; the first takes the 8-wide path, each of the others
# violates one clause of its condition
CONVERT_FIELDS = {'vec': (64, 68, 72, 0, 0), 'D%8': (60, 68, 72, 0, 0), 'ld_src%4': (64, 66, 72, 0, 0), 'ld_dst%8': (64, 68, 76, 0, 0),
                  'src_align': (64, 68, 72, 1, 0), 'dst_align': (64, 68, 72, 0, 1)}


def check_convert(b, dev, M, storage, who):
    g = torch.Generator().manual_seed(M)
    fields = [(gather_src(M, D, g), storage, ps, pd, ss, ds) for D, ps, pd, ss, ds in CONVERT_FIELDS.values()]
    vec = run_gather_multi(b, dev, fields, None, (0, 0), M, who + ' identity')
    assert vec == [storage != F32] + [False] * 5, (vec, 'each field violates exactly the clause it is meant to')


def check_convert_wrap(b, dev, storage, who):
    """(2100, 1024): 268800 chunks of 8 for 1024 x 256 = 262144 threads - the grid-stride loop takes a second trip."""
    M, D = 2100, 1024
    assert M * D // 8 == 268800 > 1024 * 256
    g = torch.Generator().manual_seed(5)
    vec = run_gather_multi(b, dev, [(gather_src(M, D, g), storage, D + 4, D + 8, 0, 0)], None, (0, 0), M, who + ' wrap')
    assert vec == [True]


# ------------------------------------------------------------------------------------------------ begin_step
def check_begin_step(b, dev, step, n_acc, absent, who):
    """absent: one of None, 'opt_state', 'acc', 'zero2', 'rng_bump'."""
    b1, b2 = 0.9, 0.999
    st0 = torch.tensor([float(step), 1e-3, b1, b2, 1e-8, 0.123, 0.456, 7.0, NAN], dtype=F64)
    st = st0.clone().to(dev)
    g = torch.Generator().manual_seed(n_acc)
    acc = torch.cat([torch.randn(n_acc, generator=g, dtype=F64), torch.full((1,), NAN, dtype=F64)]).to(dev)
    n2 = n_acc // 2 + 3
    z2 = torch.cat([torch.randn(n2, generator=g, dtype=F64), torch.full((1,), NAN, dtype=F64)]).to(dev)
    rng = torch.tensor([0x1234567, 41, SENT_I], dtype=torch.int64).to(dev)
    b.begin_step(None if absent == 'opt_state' else st[:8], None if absent == 'acc' else acc[:n_acc],
                 zero2=None if absent == 'zero2' else z2[:n2], rng_bump=None if absent == 'rng_bump' else rng[:2])
    _sync(dev)
    st, acc1, z21, rng = st.cpu(), acc.cpu(), z2.cpu(), rng.cpu()
    if absent == 'opt_state':
        same(st, st0, 'opt_state untouched')
    else:
        assert float(st[0]) == step + 1, (float(st[0]), step + 1)
        same(st[[1, 2, 3, 4, 7, 8]], st0[[1, 2, 3, 4, 7, 8]], 'opt_state: the other words')
        for slot, beta in ((5, b1), (6, b2)):
            err = abs(float(st[slot]) - (1 - beta ** (step + 1)))
            print(f'{who} begin_step step {step}: |bias_corr - (1 - {beta} ** {step + 1})| = {err:.3g} (allowed {8 * 2.0 ** -53:.3g})')
            assert err <= 8 * 2.0 ** -53, (slot, err)
    for name, t, n in (('acc', acc1, n_acc), ('zero2', z21, n2)):
        _sent(t[n:], name)
        if absent == name:
            assert bool((t[:n] != 0).all()), name + ' untouched'
        else:
            same(t[:n], torch.zeros(n, dtype=F64), name + ' zeroed')
    assert rng.tolist() == [0x1234567, 41 if absent == 'rng_bump' else 42, SENT_I], rng.tolist()
    COUNTS['sentinels'] += 1
    COUNTS['cases'] += 1


# ------------------------------------------------------------------------------------------------ Adam, axpy, clip
BETAS, EPS = (0.9, 0.999), 1e-8


def adam_ref(w, g, m, v, step, lr, dtype, betas=BETAS, eps=EPS):
    """torch/optim/adam.py _single_tensor_adam for one tensor, as restated.adam_step has its lines; `step` is the step being
    taken (after its increment).  -> (w, m, v, update)."""
    w, g, m, v = (t.to(dtype).clone() for t in (w, g, m, v))
    bc1 = 1 - betas[0] ** step
    bc2 = 1 - betas[1] ** step
    m.lerp_(g, 1 - betas[0])
    v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    w0 = w.clone()
    w.addcdiv_(m, denom, value=-lr / bc1)
    return w, m, v, w - w0


def opt_state(step, lr, betas=BETAS, eps=EPS):
    return torch.tensor([float(step), lr, betas[0], betas[1], eps, 1 - betas[0] ** step, 1 - betas[1] ** step, 0.0], dtype=F64)


def adam_case(n, step, seed=0):
    """g = N(0, 1) 10^k, k uniform in -8 .. 2 per element, m0 and v0 at matching scales; up to 100 zero gradients, half of them
    with zero moments (m / eps with m == 0); step 1 starts from zero moments."""
    g_ = torch.Generator().manual_seed(n + 7 * step + seed)
    sc = 10.0 ** torch.randint(-8, 3, (n,), generator=g_).float()
    g = torch.randn(n, generator=g_) * sc
    m = 0.3 * torch.randn(n, generator=g_) * sc
    v = (0.5 + torch.rand(n, generator=g_)) * sc * sc
    w = torch.randn(n, generator=g_)
    nz = min(100, n // 2)
    g[:nz] = 0.0
    m[:nz // 2], v[:nz // 2] = 0.0, 0.0
    if step == 1:
        m.zero_()
        v.zero_()
    return {'n': n, 'step': step, 'lr': 1e-3, 'w': w, 'g': g, 'm': m, 'v': v, 'zeros': nz}


def adam_bounds(c, r64):
    """S_m, S_v, S_w of the docstring, from the f64 run."""
    w0, g, m0 = c['w'].double(), c['g'].double(), c['m'].double()
    return m0.abs() + (1 - BETAS[0]) * (g - m0).abs(), r64[2].abs(), w0.abs() + r64[3].abs()


def check_adam(b, dev, c, who):
    n = c['n']
    tail = torch.full((1,), NAN)
    w, g, m, v = (torch.cat([c[k], tail]).to(dev) for k in 'wgmv')
    st = torch.cat([opt_state(c['step'], c['lr']), torch.full((1,), NAN, dtype=F64)]).to(dev)
    b.adam(w[:n], g[:n], m[:n], v[:n], st[:8])
    _sync(dev)
    for t in (w, g, m, v):
        _sent(t[n:], 'adam')
    same(g[:n], c['g'], 'adam leaves the gradient alone')
    same(st, torch.cat([opt_state(c['step'], c['lr']), torch.full((1,), NAN, dtype=F64)]), 'adam leaves opt_state alone')
    r64, r32 = (adam_ref(c['w'], c['g'], c['m'], c['v'], c['step'], c['lr'], dt) for dt in (F64, F32))
    Sm, Sv, Sw = adam_bounds(c, r64)
    tag = f'{who} adam n{n} step{c["step"]}'
    elem_within(m[:n], r64[1], r32[1], Sm, 3, tag + ' m', ('adam', 'm'))
    elem_within(v[:n], r64[2], r32[2], Sv, 4, tag + ' v', ('adam', 'v'))
    elem_within(w[:n], r64[0], r32[0], Sw, 8, tag + ' w', ('adam', 'w'))
    COUNTS['cases'] += 1


def axpy_ref(g, w, coef, dtype):
    return g.to(dtype) + f32(coef) * w.to(dtype)


def check_axpy(b, dev, n, coef, who):
    c = adam_case(n, 4, seed=1)
    tail = torch.full((1,), NAN)
    g, w = torch.cat([c['g'], tail]).to(dev), torch.cat([c['w'], tail]).to(dev)
    b.axpy(g[:n], w[:n], coef)
    _sync(dev)
    _sent(g[n:], 'axpy')
    same(w, torch.cat([c['w'], tail]), 'axpy leaves w alone')
    r64, r32 = axpy_ref(c['g'], c['w'], coef, F64), axpy_ref(c['g'], c['w'], coef, F32)
    elem_within(g[:n], r64, r32, c['g'].double().abs() + (f32(coef) * c['w'].double()).abs(), 2, f'{who} axpy n{n} c{coef}', ('axpy', 'g'))
    COUNTS['cases'] += 1


CLIP_N = (1, 255, 100003, 1048576 + 257)


def clip_ref(g, sqnorm, max_norm, dtype):
    """restated.clip_grad_norm's coefficient with the total norm given as its square (the kernel's operand)."""
    total = torch.sqrt(torch.tensor(sqnorm, dtype=dtype))
    coef = torch.clamp(f32(max_norm) / (total + 1e-6), max=1.0)
    return g.to(dtype) * coef, coef


def check_clip_scale(b, dev, n, kind, who):
    """kind: 'above' / 'below' (the true squared norm against max_norm), 'zero', 'inf', 'nan' (that squared norm given)."""
    g_ = torch.Generator().manual_seed(n)
    g0 = torch.randn(n, generator=g_)
    true = float((g0.double() ** 2).sum())
    sq = {'above': true, 'below': true, 'zero': 0.0, 'inf': float('inf'), 'nan': NAN}[kind]
    max_norm = 2.0 * math.sqrt(true) if kind == 'below' else 0.37 * math.sqrt(true)
    g = torch.cat([g0, torch.full((1,), NAN)]).to(dev)
    acc = torch.tensor([NAN, NAN, sq, NAN], dtype=F64).to(dev)
    b.clip_scale(g[:n], acc, 2, max_norm)
    _sync(dev)
    _sent(g[n:], 'clip_scale')
    same(acc, torch.tensor([NAN, NAN, sq, NAN], dtype=F64), 'clip_scale leaves its operand alone')
    (r64, c64), (r32, _) = clip_ref(g0, sq, max_norm, F64), clip_ref(g0, sq, max_norm, F32)
    if kind in ('below', 'zero'):
        assert float(c64) == 1.0
        same(g[:n], g0, 'a norm under the bound leaves the buffer bitwise')
    if kind == 'nan':
        assert bool(torch.isnan(r64).all())
    if kind == 'inf':
        assert float(c64) == 0.0
    within(g[:n], r64, r32, f'{who} clip_scale n{n} {kind}', key=('clip_scale', 'g'))
    COUNTS['cases'] += 1
    COUNTS['elements'] += n


# ------------------------------------------------------------------------------------------------ apply_multi
def _fbits(x):
    return struct.unpack('<i', struct.pack('<f', x))[0]


def layer_spec(n, k, ss, sd, coef, sa, sb, wide, bias=True):
    return dict(n=n, k=k, ss=ss, sd=sd, coef=coef, sa=sa, sb=sb, wide=wide, bias=bias)


# every spec of tests/test_gpu_ops.py::test_apply_multi_fused_optimizer_step, kept
OLD_SPECS = [layer_spec(*s) for s in ((48, 53, 37, 64, 0.02, 3, 5, 0), (130, 200, 200, 200, 0.0, -1, -1, 0), (1, 70, 70, 70, 0.5, 4, -1, 0),
                                      (130, 200, 200, 200, 0.0, -1, -1, 1), (300, 520, 256, 264, 0.01, 6, 7, 1), (31, 512, 512, 512, 0.0, -1, -1, 1))]


def apply_tiles(s):
    """Tiles of one layer: 32 x 128 on the wide path, 32 x 32 on the scalar path; the grid has 256 workgroups per layer."""
    return ((s['k'] + 127) // 128 if s['wide'] else (s['k'] + 31) // 32) * ((s['n'] + 31) // 32)


def apply_plans():
    """name -> list of layers of ONE launch."""
    P = {'old': OLD_SPECS,
         'second_trip_scalar': [layer_spec(264, 1060, 1060, 1060, 0.01, 2, -1, 0)],
         'second_trip_wide': [layer_spec(264, 4100, 4096, 4104, 0.0, 1, 2, 1)],
         # two layers into one slot; A only; none
         'slots': [layer_spec(33, 40, 40, 40, 0.02, 3, 4, 0), layer_spec(17, 132, 64, 72, 0.03, 3, -1, 1), layer_spec(16, 36, 36, 36, 0.0, -1, -1, 0)],
         'no_bias': [layer_spec(15, 124, 124, 124, 0.01, 5, 6, 1, bias=False), layer_spec(31, 35, 20, 23, 0.0, 6, -1, 0, bias=False)]}
    P['n_real'] = [layer_spec(n, 132 if i % 2 else 124, 64 if i % 2 else 124, 72 if i % 2 else 124, 0.01 * (i % 3), i % 4, -1, 1)
                   for i, n in enumerate((1, 15, 16, 17, 31, 33, 48))]
    P['n_real_scalar'] = [layer_spec(n, 37, 30, 33, 0.01 * (i % 3), 7, -1, 0) for i, n in enumerate((1, 15, 16, 17, 31, 33, 48))]
    P['k4'] = [layer_spec(33, 4, 4, 4, 0.5, 0, 1, 1), layer_spec(48, 132, 4, 12, 0.0, 2, 3, 1), layer_spec(16, 4, 4, 4, 0.0, 4, 5, 1),
               layer_spec(31, 32, 32, 32, 0.0, 6, 7, 0)]        # (the last two: one tile, one contribution per slot)
    return P


def apply_case(specs, seed=0):
    """Per layer: W, g, m, v [n, k] and the bias quadruple, gradients from the family of adam_case (reshaped)."""
    g = torch.Generator().manual_seed(len(specs) + seed)
    out = []
    for i, s in enumerate(specs):
        n, k = s['n'], s['k']
        a = adam_case(n * k, 4, seed=seed + i)
        bq = adam_case(n, 4, seed=seed + 100 + i)
        L = {kk: a[kk].view(n, k) for kk in 'wgmv'}
        L.update({'b' + kk: bq[kk] for kk in 'wgmv'})
        out.append(L)
    return out


def apply_ref(s, L, step, lr, dtype):
    """One layer: the exported gradient g + c w0 (learning/ase_agent.py's weight-only loss terms through autograd), Adam on it,
    Adam on the bias with its own gradient."""
    coef = f32(s['coef'])
    gx = L['g'].to(dtype) + coef * L['w'].to(dtype) if coef != 0 else L['g'].to(dtype)
    w, m, v, up = adam_ref(L['w'], gx, L['m'], L['v'], step, lr, dtype)
    bw, bm, bv, bup = adam_ref(L['bw'], L['bg'], L['bm'], L['bv'], step, lr, dtype)
    return {'g': gx, 'w': w, 'm': m, 'v': v, 'up': up, 'bw': bw, 'bm': bm, 'bv': bv, 'bup': bup}


def _odd(x, dev):
    """x at an odd 4-byte offset of its buffer, one NaN word before and after."""
    flat = torch.full((x.numel() + 2,), NAN)
    flat[1:-1] = x.reshape(-1)
    flat = flat.to(dev)
    return flat, flat[1:-1].view(x.shape)


def run_apply(b, dev, specs, case, storage, step=4, lr=1e-3, with_state=True, split=None):
    n_slots = 8
    acc = torch.full((n_slots + 1,), ACC0, dtype=F64)
    acc[n_slots] = NAN
    acc = acc.to(dev)
    st = opt_state(step, lr).to(dev) if with_state else None
    rows, items, keep = [], [], []
    for s, L in zip(specs, case):
        n, k, gap = s['n'], s['k'], s['sd'] - s['ss']
        T = {kk: _odd(L[kk], dev) for kk in 'wgmv'}
        B = {kk: _odd(L['b' + kk], dev) for kk in 'wgmv'}
        ldws, ldwts = (k + gap + 3) // 4 * 4 + 8, (n + 3) // 4 * 4 + 4
        Ws, Wts = nanbuf((n + 1, ldws), dev, storage), nanbuf((k + gap + 1, ldwts), dev, storage)
        bs = nanbuf((n + 1,), dev)
        if s['wide']:
            assert k % 4 == 0 and s['ss'] % 4 == 0 and gap % 4 == 0 and ldws % 4 == 0 and ldwts % 4 == 0
        hb = s['bias']
        rows.append([T['w'][1].data_ptr(), n, k, Ws.data_ptr(), ldws, Wts.data_ptr(), ldwts, s['ss'], gap,
                     B['w'][1].data_ptr() if hb else 0, bs.data_ptr() if hb else 0, (k + 31) // 32, T['g'][1].data_ptr(), T['m'][1].data_ptr(),
                     T['v'][1].data_ptr(), B['g'][1].data_ptr(), B['m'][1].data_ptr(), B['v'][1].data_ptr(), _fbits(s['coef']), s['sa'], s['sb'],
                     s['wide'], 0, 0])
        items.append((T['w'][1], Ws[:n], Wts[:k + gap, :n], s['ss'], s['sd'], B['w'][1] if hb else None, bs[:n], T['g'][1], T['m'][1], T['v'][1], B['g'][1],
                      B['m'][1], B['v'][1], s['coef'], s['sa'], s['sb']))
        keep.append({'T': T, 'B': B, 'Ws': Ws, 'Wts': Wts, 'bs': bs})
    desc = torch.tensor(rows, dtype=torch.int64).to(dev)
    if split is not None:
        split(b, desc, items, storage, st, acc[:n_slots], keep)
    else:
        b.apply_multi(desc, items, storage, st, acc[:n_slots])
    _sync(dev)
    return keep, acc.cpu()


def check_apply(b, dev, specs, case, storage, who, step=4, lr=1e-3, with_state=True, split=None, name=''):
    keep, acc = run_apply(b, dev, specs, case, storage, step, lr, with_state, split)
    _sent(acc[8:], 'acc')
    want = {}
    for li, (s, L, K) in enumerate(zip(specs, case, keep)):
        n, k, gap, ss = s['n'], s['k'], s['sd'] - s['ss'], s['ss']
        tag = f'{who} apply_multi {name}[{li}] {n}x{k} wide={s["wide"]} {_name(storage)}'
        got = {kk: K['T'][kk][1].cpu() for kk in 'wgmv'}
        gotb = {kk: K['B'][kk][1].cpu() for kk in 'wgmv'}
        for grp in (K['T'], K['B']):
            for flat, _ in grp.values():
                f = flat.cpu()
                assert f[0] != f[0] and f[-1] != f[-1], (tag, 'the words around a flat tensor')
                COUNTS['sentinels'] += 2
        if not with_state:
            for kk in 'wgmv':
                same(got[kk], L[kk], tag + ' without opt_state: ' + kk + ' untouched')
                same(gotb[kk], L['b' + kk], tag + ' without opt_state: bias ' + kk + ' untouched')
        else:
            r64, r32 = apply_ref(s, L, step, lr, F64), apply_ref(s, L, step, lr, F32)
            key = ('apply_multi',)
            g0, w0, m0 = L['g'].double(), L['w'].double(), L['m'].double()
            if f32(s['coef']) != 0:
                elem_within(got['g'], r64['g'], r32['g'], g0.abs() + (f32(s['coef']) * w0).abs(), 2, tag + ' exported g', key + ('g',))
            else:
                same(got['g'], L['g'], tag + ' coefficient 0: g untouched')
            elem_within(got['m'], r64['m'], r32['m'], m0.abs() + (1 - BETAS[0]) * (r64['g'] - m0).abs(), 3, tag + ' m', key + ('m',))
            elem_within(got['v'], r64['v'], r32['v'], r64['v'].abs(), 4, tag + ' v', key + ('v',))
            elem_within(got['w'], r64['w'], r32['w'], w0.abs() + r64['up'].abs(), 8, tag + ' w', key + ('w',))
            same(gotb['g'], L['bg'], tag + ' bias gradient untouched')
            if s['bias']:
                bm0 = L['bm'].double()
                elem_within(gotb['m'], r64['bm'], r32['bm'], bm0.abs() + (1 - BETAS[0]) * (L['bg'].double() - bm0).abs(), 3, tag + ' bias m', key + ('bias m',))
                elem_within(gotb['v'], r64['bv'], r32['bv'], r64['bv'].abs(), 4, tag + ' bias v', key + ('bias v',))
                elem_within(gotb['w'], r64['bw'], r32['bw'], L['bw'].double().abs() + r64['bup'].abs(), 8, tag + ' bias', key + ('bias',))
            else:
                for kk in 'wmv':
                    same(gotb[kk], L['b' + kk], tag + ' no bias: ' + kk + ' untouched')
            for slot in {s['sa'], s['sb'] if s['sa'] >= 0 else -1} - {-1}:
                want.setdefault(slot, []).append((L['w'].double() ** 2).reshape(-1, 1))
        # the shadows: bitwise the conversion of what the kernel itself stored
        cols = torch.tensor([j if j < ss else j + gap for j in range(k)])
        Ws, Wts, bs = K['Ws'].cpu(), K['Wts'].cpu(), K['bs'].cpu()
        cv = convert(got['w'], storage)
        same(Ws[:n][:, cols], cv, tag + ' W_s')
        same(Wts[cols][:, :n], cv.t().contiguous(), tag + ' W_s^T')
        m = torch.ones(Ws.shape, dtype=torch.bool)
        m[:n, cols] = False
        _sent(Ws[m], tag + ' W_s gap / pad / rows past n_real')
        m = torch.ones(Wts.shape, dtype=torch.bool)
        m[cols, :n] = False
        _sent(Wts[m], tag + ' W_s^T gap / pad')
        if s['bias']:
            same(bs[:n], gotb['w'], tag + ' bias copy')
            _sent(bs[n:], tag + ' bias copy')
        else:
            _sent(bs, tag + ' no bias: no copy')
    for s in specs:                    # one workgroup's contribution into each: slot B is bitwise slot A
        if with_state and s['sa'] >= 0 and s['sb'] >= 0 and apply_tiles(s) == 1 and len(want[s['sa']]) == len(want[s['sb']]) == 1:
            same(acc[s['sb']], acc[s['sa']], f'{name}: slot B is bitwise slot A')
    for slot in range(8):
        if slot in want:
            sum_bound(acc[slot:slot + 1], torch.cat(want[slot]), f'{who} apply_multi {name} slot {slot}', ('apply_multi', 'w2'))
        else:
            assert float(acc[slot]) == ACC0, (name, 'foreign slot', slot)
    COUNTS['cases'] += 1
    return keep, acc
