"""tests/ref_update.py pinned without a GPU: the emulator (tests/emu_backend.py) run over every case of
tests/test_gpu_update.py and held to the same bounds - so cases and bounds are satisfiable; the fixtures' own conditions (every
case reaches the kernel path it is meant for, the tile and chunk counts, the special elements); thirteen single-term wrong
restatements of the emulator, each of which must fail a bound on the committed cases - so the bounds have teeth; and the Adam
restatement held torch.equal to torch.optim.Adam itself."""
import inspect
import textwrap

import pytest
import torch

from ase_amd import lib as L
from oracle import restated as R
from tests import emu_backend
from tests import ref_update as RU
from tests.emu_gp_fuse import FusedEmuBackend

F32, F64 = RU.F32, RU.F64
ST_IDS = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}
DEV = 'cpu'


@pytest.fixture(scope='module')
def emu():
    return FusedEmuBackend()


def test_storage_codes_are_the_library_s():
    assert RU.CODE == {torch.bfloat16: L.BF16, torch.float32: L.F32, torch.float16: L.F16}


# ------------------------------------------------------------------------------------------------ the emulator on every case
def test_emulator_moments(emu):
    for c, multi in RU.moments_plan():
        RU.check_moments(emu, DEV, c, 'emu', multi)
        if multi:                                          # the 1 / 3 / 4-stream launch against single launches
            RU.check_moments(emu, DEV, c, 'emu', False)


def test_emulator_finalize(emu):
    for c, multi in RU.finalize_plan():
        RU.check_finalize(emu, DEV, c, 'emu', multi)
    for fam in RU.FAMILIES:
        RU.check_halves(emu, DEV, RU.rms_case(129, 260, 'wide', fam, seed=23), 'emu')
        RU.check_halves(emu, DEV, RU.rms_case(65, 3, 'wide', fam, seed=23), 'emu')
    for D in (3, 260, 1400):
        RU.check_eval(emu, DEV, RU.rms_case(65, D, 'wide', 'warm'), 'emu')


@pytest.mark.parametrize('st', RU.STORAGES, ids=ST_IDS.values())
def test_emulator_normalize(emu, st):
    for kw in RU.normalize_plan():
        RU.check_normalize(emu, DEV, RU.norm_case(**kw), st, 'emu')


def test_emulator_unnormalize(emu):
    for n in RU.UNNORM_N:
        RU.check_unnormalize(emu, DEV, RU.unnorm_case(n), 'emu')


@pytest.mark.parametrize('st', RU.STORAGES, ids=ST_IDS.values())
def test_emulator_gather(emu, st):
    for M in RU.GATHER_M:
        for D in RU.GATHER_D:
            RU.check_gather_rows(emu, DEV, M, D, st, 'emu')
    for M in (1, 15, 16, 17, 300):
        RU.check_gather_multi(emu, DEV, M, 'emu', rot=RU.STORAGES.index(st))
        RU.check_convert(emu, DEV, M, st, 'emu')
    if st != F32:
        RU.check_convert_wrap(emu, DEV, st, 'emu')


def test_emulator_begin_step(emu):
    for step in (0, 1, 999, 99999):
        for n_acc in (1, 1024, 1025, 3000):
            RU.check_begin_step(emu, DEV, step, n_acc, None, 'emu')
    for absent in ('opt_state', 'acc', 'zero2', 'rng_bump'):
        RU.check_begin_step(emu, DEV, 999, 1025, absent, 'emu')


def test_emulator_adam_axpy_clip(emu):
    for n in (1, 255, 100003):
        for step in (1, 4, 1000):
            RU.check_adam(emu, DEV, RU.adam_case(n, step), 'emu')
        for coef in (0.02, 0.0):
            RU.check_axpy(emu, DEV, n, coef, 'emu')
    RU.check_adam(emu, DEV, RU.adam_case(4096 * 256 + 1, 4), 'emu')
    for n in RU.CLIP_N:
        for kind in ('above', 'below', 'zero', 'inf', 'nan'):
            RU.check_clip_scale(emu, DEV, n, kind, 'emu')


@pytest.mark.parametrize('st', RU.STORAGES, ids=ST_IDS.values())
def test_emulator_apply_multi(emu, st):
    for name, specs in RU.apply_plans().items():
        case = RU.apply_case(specs)
        RU.check_apply(emu, DEV, specs, case, st, 'emu', name=name)
    specs = RU.apply_plans()['slots']
    RU.check_apply(emu, DEV, specs, RU.apply_case(specs), st, 'emu', with_state=False, name='no opt_state')
    RU.check_apply(emu, DEV, specs, RU.apply_case(specs), st, 'emu', step=1, name='step 1')


# ------------------------------------------------------------------------------------------------ the fixtures' conditions
def test_fixture_conditions():
    # moments: both kernels are reached by every way the issue names (the check bodies assert case['wide'] against the entry's
    # condition on the tensors they launch with)
    plan = RU.moments_plan()
    wide = {(c['M'], c['D']) for c, _ in plan if c['streams'][0]['wide']}
    assert {(M, D) for M in RU.RMS_M for D in (4, 64, 260)} <= wide
    for path in RU.RMS_PATHS:
        cs = [c for c, _ in plan if c['streams'][0]['path'] == path]
        assert cs and all(c['streams'][0]['wide'] == (path in ('wide', 'remap') and c['D'] % 4 == 0) for c in cs), path
    assert any(c['streams'][0]['wide'] and c['streams'][0]['remap'][0] > 0 for c, _ in plan)       # remap without idx, 16-byte kernel
    assert any(not c['streams'][0]['wide'] and c['streams'][0]['remap'][0] > 0 and c['streams'][0]['idx'] is None for c, _ in plan)
    dup = [c for c, _ in plan if c['streams'][0]['path'] == 'dup']
    assert all(len(set(c['streams'][0]['idx'].tolist())) < c['M'] for c in dup)
    assert any((c['D'] + 3) // 4 > 64 for c in [c for c, _ in plan if c['streams'][0]['wide']])    # a second column tile (D >= 260)
    assert {len(c['streams']) for c, m in plan if m} == {1, 3, 4}
    assert {RU.finalize_threads(c['D']) for c, _ in RU.finalize_plan()} == {256, 1024}
    assert RU.finalize_threads(260) == 1024 and RU.finalize_threads(253) == 256
    # normalise: every kernel at every storage, the specials present
    kws = RU.normalize_plan()
    assert {k['kernel'] for k in kws} == set(RU.NORM_KERNELS) and {k['n_out'] for k in kws} == {1, 2, 3}
    assert any(k['D'] == 257 and k['kernel'] == 'scalar' for k in kws)                             # the scalar kernel's second column block
    c = RU.norm_case(300, 260, 'wide', 3)
    r = RU.normalize_ref(c, F64)
    for rows in (c['x'][0], c['x'][-1], c['x'][:, -1]):
        assert bool(torch.isnan(rows).any()) and float('inf') in rows and float('-inf') in rows and 100.0 in rows and -100.0 in rows
    assert bool(((c['x'] == 2.5) & (r == 5.0)).any()) and bool(((c['x'] == -2.5) & (r == -5.0)).any())
    assert float(c['std'][1]) == RU.f32(1e-5 ** 0.5)
    assert bool(torch.isnan(r[0]).any()) and bool((r[c['x'] == float('inf')] == 5).all()) and bool((r[c['x'] == float('-inf')] == -5).all())
    # gather: every lane-group width; the identity map's clauses; the wrap
    assert {RU.gather_width(D) for D in RU.GATHER_D} == {1, 2, 4, 32, 64}
    assert {RU.gather_width(D) for D in (5, 9, 17)} == {8, 16, 32}
    assert 2100 * 1024 // 8 == 268800 and 268800 > 1024 * 256
    assert RU.UNNORM_N[-1] > 2048 * 256 and RU.CLIP_N[-1] > 4096 * 256
    # apply_multi: the tile counts of the issue; every n_real of the transposed store's halves
    P = RU.apply_plans()
    assert RU.apply_tiles(P['second_trip_scalar'][0]) == 306 and RU.apply_tiles(P['second_trip_wide'][0]) == 297
    assert max(RU.apply_tiles(s) for s in P['old']) == 50 and max(RU.apply_tiles(s) for s in P['old'] if not s['wide']) == 35
    assert [s['n'] for s in P['n_real']] == [1, 15, 16, 17, 31, 33, 48] and all(s['wide'] for s in P['n_real'])
    assert {s['k'] for s in P['n_real'] + P['k4']} >= {4, 124, 132}
    assert any(s['ss'] == s['k'] and s['wide'] for s in P['n_real']) and any(s['ss'] < s['k'] and s['wide'] for s in P['n_real'])
    assert any(not s['bias'] for s in P['no_bias'])
    c = RU.adam_case(100003, 4)
    assert int((c['g'] == 0).sum()) >= 100 and int(((c['g'] == 0) & (c['m'] == 0) & (c['v'] == 0)).sum()) >= 50
    assert float(c['g'].abs().max()) > 10 and float(c['g'][c['g'] != 0].abs().min()) < 1e-8


# ------------------------------------------------------------------------------------------------ the bounds have teeth
def _wrong(method, *edits, base=FusedEmuBackend):
    """A backend whose `method` is the emulator's with single terms restated wrongly."""
    src = textwrap.dedent(inspect.getsource(getattr(emu_backend.EmuBackend, method)))
    for old, new in edits:
        assert src.count(old) >= 1, (method, old)
        src = src.replace(old, new)
    ns = dict(vars(emu_backend))
    exec(src, ns)
    return type('Wrong', (base,), {method: ns[method]})()


def _caught(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _fin(b):
    return sum(_caught(lambda c=c, m=m: RU.check_finalize(b, DEV, c, 'wrong', m)) for c, m in RU.finalize_plan())


def _app(b, names=('old', 'slots', 'n_real')):
    P = RU.apply_plans()
    return sum(_caught(lambda n=n: RU.check_apply(b, DEV, P[n], RU.apply_case(P[n]), F32, 'wrong', name=n)) for n in names)


def _ordered(*order):
    """The emulator's apply_multi with its three steps of the optimizer branch in the given order."""
    class Ordered(FusedEmuBackend):
        def apply_multi(self, desc, items, dtype, opt_state, acc):
            for (W, ws, wts, ss, sd, b, bs, gW, mW, vW, gb, mb, vb, coef, slot_a, slot_b) in items:
                def w2():
                    if slot_a >= 0:
                        s2 = (W.double() ** 2).sum()
                        acc[slot_a] += s2
                        if slot_b >= 0:
                            acc[slot_b] += s2
                steps = {'w2': w2, 'term': lambda: self.axpy(gW, W, coef) if coef != 0 else None,
                         'adam': lambda: self.adam(W, gW, mW, vW, opt_state)}
                for k in order:
                    steps[k]()
                if b is not None:
                    self.adam(b, gb, mb, vb, opt_state)
                self.refresh_shadow(W, ws, wts, ss, sd)
                if b is not None:
                    bs[:b.numel()] = b
    return Ordered()


def test_wrong_restatements_are_caught(monkeypatch):
    n_fin = len(RU.finalize_plan())
    # 1. biased variance
    assert _fin(_wrong('rms_finalize', ('/ (n - 1.0))', '/ n)'))) >= n_fin // 3
    # 2. the delta^2 term dropped (the families whose batch mean is 1e3 from the previous one)
    assert _fin(_wrong('rms_finalize', (' + delta * delta * cnt * n / tot', ''))) >= n_fin // 4
    # 3. the second stream's shift taken from the already-merged mean: every case with more than one stream whose mean moves (the
    # warm family's, 1e6 rows behind it, moves by less than an f32 ulp of 1e3)
    multi = sum(len(c['streams']) > 1 for c, _ in RU.finalize_plan())
    moving = sum(len(c['streams']) > 1 and c['family'] != 'warm' for c, _ in RU.finalize_plan())
    assert _fin(_wrong('rms_finalize', ('bm = (shift + s1 / n)', 'bm = (mean.float().double() + s1 / n)'))) == moving >= 9
    # 4. the count advanced once for three streams
    assert _fin(_wrong('rms_finalize', ('= mean, var, cnt', '= mean, var, state[2 * D] + float(count)'))) == multi
    # 5. sqrt(var) + 1e-5
    assert _fin(_wrong('rms_finalize', ('torch.sqrt(var.float() + 1e-5)', 'torch.sqrt(var.float()) + 1e-5'))) >= n_fin // 3
    # 6. a clamp that drops NaN
    b = _wrong('rms_normalize', ('torch.clamp((x - mean[:D]) / std[:D], -5.0, 5.0)',
                                 'torch.nan_to_num(torch.clamp((x - mean[:D]) / std[:D], -5.0, 5.0), nan=-5.0)'))
    kws = RU.normalize_plan()
    assert sum(_caught(lambda kw=kw: RU.check_normalize(b, DEV, RU.norm_case(**kw), F32, 'wrong')) for kw in kws) == len(kws)
    # 7. the remap's two factors exchanged
    wrong_rows = dict(vars(emu_backend))
    src = inspect.getsource(emu_backend._rows)
    assert src.count('H, N = remap') == 1
    exec(src.replace('H, N = remap', 'N, H = remap'), wrong_rows)
    remapped = [(c, m) for c, m in RU.moments_plan() if c['streams'][0]['remap'][0] > 0 and c['M'] > 2]
    with monkeypatch.context() as mp:
        mp.setattr(emu_backend, '_rows', wrong_rows['_rows'])
        assert sum(_caught(lambda c=c, m=m: RU.check_moments(FusedEmuBackend(), DEV, c, 'wrong', m)) for c, m in remapped) == len(remapped)
    # 8. Adam with bc2 outside the square root; 9. eps added before the division by sqrt(bc2)
    cases = [RU.adam_case(100003, step) for step in (1, 4, 1000)]
    for edit in (('torch.tensor(math.sqrt(s[6])).float()', 'torch.tensor(s[6]).float()'),
                 ('denom = v.sqrt() / bc2s + eps', 'denom = (v.sqrt() + eps) / bc2s')):
        b = _wrong('adam', edit)
        assert sum(_caught(lambda c=c: RU.check_adam(b, DEV, c, 'wrong')) for c in cases) == 3
    # 10. the weight term added after Adam instead of into the exported gradient; 11. w^2 of the post-update weights (the
    # emulator's three steps in another order; in its own order the variant passes)
    assert _app(_ordered('w2', 'term', 'adam')) == 0
    assert _app(_ordered('w2', 'adam', 'term')) == 3
    assert _app(_ordered('term', 'adam', 'w2'), ('old', 'slots')) == 2
    # 12. slot B ignored
    assert _app(_wrong('apply_multi', ('acc[slot_b] += s2', 'pass')), ('old', 'k4')) == 2
    # 13. the bias stepped with lr instead of lr / bc1
    b = _wrong('apply_multi', ('self.adam(b, gb, mb, vb, opt_state)',
                               'self.adam(b, gb, mb, vb, torch.cat([opt_state[:5], torch.ones(1, dtype=opt_state.dtype), opt_state[6:]]))'))
    assert _app(b) == 3


# ------------------------------------------------------------------------------------------------ the restatements are the reference's
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_adam_restatement_is_torch_optim_adam(dtype):
    g_ = torch.Generator().manual_seed(4)
    w0 = torch.randn(1000, generator=g_).to(dtype)
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.Adam([p], lr=1e-3, betas=RU.BETAS, eps=RU.EPS, foreach=False)
    w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
    for step in (1, 2, 3):
        g = (torch.randn(1000, generator=g_) * 10.0 ** torch.randint(-8, 3, (1000,), generator=g_)).to(dtype)
        p.grad = g.clone()
        opt.step()
        w, m, v, _ = RU.adam_ref(w, g, m, v, step, 1e-3, dtype)
        assert torch.equal(p.detach(), w) and torch.equal(opt.state[p]['exp_avg'], m) and torch.equal(opt.state[p]['exp_avg_sq'], v), step


def test_clip_restatement_is_restated_clip_grad_norm():
    g = torch.randn(1000, generator=torch.Generator().manual_seed(2), dtype=F64)
    for max_norm in (0.5, 100.0):
        p = torch.nn.Parameter(torch.zeros(1000, dtype=F64))
        p.grad = g.clone()
        total = R.clip_grad_norm({'p': p}, RU.f32(max_norm))
        want, _ = RU.clip_ref(g, float(total) ** 2, max_norm, F64)
        assert float((p.grad - want).abs().max()) <= 4 * 2.0 ** -53 * float(g.abs().max())
