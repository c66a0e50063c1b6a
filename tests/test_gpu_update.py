"""The running-statistics, gather and optimizer kernels (csrc/rms.hip, csrc/optim.hip) on the MI355X against
tests/ref_update.py: the reference's own expressions in f64 (oracle/restated.py, torch's .to(dtype)) - NOT the emulator, which
tests/test_update_ref.py holds to the same cases and bounds on the CPU.  Every output lives inside a larger NaN-filled
allocation with a row pitch wider than its payload; every sentinel is checked after each launch; the bounds are derived in
tests/ref_update.py.

The cases that failed on the previous library (8 tests; run once against each library): test_normalize[f32], [bf16], [f16]
and test_unnormalize - fminf / fmaxf turned a NaN observation into -5 (and IEEE half storage went through the saturating
conversion) - and test_clip_scale[1-nan], [255-nan], [100003-nan], [1048833-nan] - a NaN norm gave the coefficient 1 and left
the gradients as they were.  The other 60 tests pass on both."""
import json
import os

import pytest
import torch

from tests import ref_update as RU

pytestmark = pytest.mark.gpu

ST_IDS = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}
DEV = 'cuda'


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    yield HipBackend()
    out = os.environ.get('ASE_UPDATE_REPORT')            # the observed deviations beside e_ref, for COVERAGE.md
    if out:
        stats = {' | '.join(k): v for k, v in sorted(RU.STATS.items()) if k[0] in RU.OPS}
        with open(out, 'w') as f:
            json.dump({'stats': stats, 'counts': RU.COUNTS}, f, indent=1)


def test_moments(be):
    for c, multi in RU.moments_plan():
        got = RU.check_moments(be, DEV, c, 'hip', multi)
        if multi:                                          # the 1 / 3 / 4-stream launch against single launches
            one = RU.check_moments(be, DEV, c, 'hip', False)
            if c['M'] <= 64:                               # one row block per column: one addition into each slot, no order left
                RU.same(got, one, 'rms_moments_multi against single launches')


def test_finalize(be):
    for c, multi in RU.finalize_plan():
        RU.check_finalize(be, DEV, c, 'hip', multi)


def test_finalize_two_halves_and_eval(be):
    for fam in RU.FAMILIES:
        RU.check_halves(be, DEV, RU.rms_case(129, 260, 'wide', fam, seed=23), 'hip')
        RU.check_halves(be, DEV, RU.rms_case(65, 3, 'wide', fam, seed=23), 'hip')
    for D in (3, 260, 1400):
        RU.check_eval(be, DEV, RU.rms_case(65, D, 'wide', 'warm'), 'hip')


@pytest.mark.parametrize('st', RU.STORAGES, ids=ST_IDS.values())
def test_normalize(be, st):
    for kw in RU.normalize_plan():
        RU.check_normalize(be, DEV, RU.norm_case(**kw), st, 'hip')


def test_unnormalize(be):
    for n in RU.UNNORM_N:
        RU.check_unnormalize(be, DEV, RU.unnorm_case(n), 'hip')


@pytest.mark.parametrize('st', RU.STORAGES, ids=ST_IDS.values())
def test_gather_rows(be, st):
    for M in RU.GATHER_M:
        for D in RU.GATHER_D:
            RU.check_gather_rows(be, DEV, M, D, st, 'hip')


@pytest.mark.parametrize('st', RU.STORAGES, ids=ST_IDS.values())
def test_gather_multi_and_convert(be, st):
    for M in (1, 15, 16, 17, 300):
        RU.check_gather_multi(be, DEV, M, 'hip', rot=RU.STORAGES.index(st))
        RU.check_convert(be, DEV, M, st, 'hip')
    if st != torch.float32:
        RU.check_convert_wrap(be, DEV, st, 'hip')


def test_begin_step(be):
    for step in (0, 1, 999, 99999):
        for n_acc in (1, 1024, 1025, 3000):
            RU.check_begin_step(be, DEV, step, n_acc, None, 'hip')
    for absent in ('opt_state', 'acc', 'zero2', 'rng_bump'):
        RU.check_begin_step(be, DEV, 999, 1025, absent, 'hip')


@pytest.mark.parametrize('step', (1, 4, 1000))
def test_adam(be, step):
    for n in (1, 255, 100003) + ((4096 * 256 + 1,) if step == 4 else ()):
        RU.check_adam(be, DEV, RU.adam_case(n, step), 'hip')


def test_axpy(be):
    for n in (1, 255, 100003):
        for coef in (0.02, 0.0):
            RU.check_axpy(be, DEV, n, coef, 'hip')


@pytest.mark.parametrize('kind', ('above', 'below', 'zero', 'inf', 'nan'))
@pytest.mark.parametrize('n', RU.CLIP_N)
def test_clip_scale(be, n, kind):
    RU.check_clip_scale(be, DEV, n, kind, 'hip')


@pytest.mark.parametrize('st', RU.STORAGES, ids=ST_IDS.values())
@pytest.mark.parametrize('name', list(RU.apply_plans()))
def test_apply_multi(be, name, st):
    specs = RU.apply_plans()[name]
    RU.check_apply(be, DEV, specs, RU.apply_case(specs), st, 'hip', name=name)


@pytest.mark.parametrize('st', RU.STORAGES, ids=ST_IDS.values())
def test_apply_multi_shadows_only_and_first_step(be, st):
    specs = RU.apply_plans()['slots']
    RU.check_apply(be, DEV, specs, RU.apply_case(specs), st, 'hip', with_state=False, name='no opt_state')
    RU.check_apply(be, DEV, specs, RU.apply_case(specs), st, 'hip', step=1, name='step 1')


@pytest.mark.parametrize('name', ('slots', 'n_real', 'n_real_scalar'))
def test_apply_multi_v2_first_pair_is_apply_multi(be, name):
    """ase_hip_apply_multi_v2 (IEEE half storage) with no second shadow pair in any row: every tensor of the first pair, the
    parameters and the moments bitwise those of ase_hip_apply_multi (tests/test_gpu_gp_fuse.py pins the second pair)."""
    specs = RU.apply_plans()[name]
    case = RU.apply_case(specs)

    def split(b, desc, items, storage, st, acc, keep):
        d2 = torch.zeros(desc.shape[0], 8, dtype=torch.int64, device=desc.device)
        b.apply_multi_split(desc, items, storage, st, acc, d2, [None] * desc.shape[0])
    k2, _ = RU.check_apply(be, DEV, specs, case, torch.float16, 'hip v2', split=split, name=name)
    k1, _ = RU.check_apply(be, DEV, specs, case, torch.float16, 'hip', name=name)
    for a, b in zip(k1, k2):
        for kk in 'wgmv':
            RU.same(a['T'][kk][0], b['T'][kk][0], 'v2 ' + kk)
            RU.same(a['B'][kk][0], b['B'][kk][0], 'v2 bias ' + kk)
        for kk in ('Ws', 'Wts', 'bs'):
            RU.same(a[kk], b[kk], 'v2 ' + kk)
