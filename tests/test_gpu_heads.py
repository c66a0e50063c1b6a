"""The loss-head kernels (csrc/heads.hip) on the MI355X against tests/ref_heads.py: f64 autograd of the reference's own forward
expressions - NOT the emulator, which tests/test_heads_ref.py holds to the same cases and bounds on the CPU.  Every output lives
inside a larger NaN-filled allocation with a row pitch wider than its payload; every sentinel is checked after each launch.
Stored gradients: max |hip - f64| <= 2 e_ref + one f32 ulp of the largest magnitude (+ half a storage ulp); loss sums: the sum
bound; bias gradients: the column sums of what was stored; counts exact (the bounds are derived in tests/ref_heads.py).

The cases that failed on the previous library (13 tests): finalize_scalars with has_div and masked == 0 reported ACC_DIV /
acc[MASK_SUM] where the gradient of ppo_head divides by m_global (test_finalize_scalars[0-*-*-1]); the NaN-row cases of
ppo_head (fmaxf / fminf dropped the NaN from the surrogate, the bound and diversity losses and the diversity rows' gradient);
enc_out of a row with one NaN (test_enc_heads).  The 1e-20 row of enc_gp_back (J = 0 on F.normalize's floor) was fixed with
them."""
import json
import os

import pytest
import torch

from tests import ref_heads as RH

pytestmark = pytest.mark.gpu

ST_IDS = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}
PPO = [(pid, mk, st) for pid, mk, sts in RH.ppo_plan() for st in sts]
DEV = 'cuda'


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    yield HipBackend()
    out = os.environ.get('ASE_HEADS_REPORT')             # the observed deviations beside e_ref, for COVERAGE.md
    if out:
        with open(out, 'w') as f:
            json.dump({' | '.join(k): v for k, v in sorted(RH.STATS.items())}, f, indent=1)


@pytest.mark.parametrize('pid,mk,st', PPO, ids=[f'{p}-{ST_IDS[s]}' for p, _, s in PPO])
def test_ppo_head(be, pid, mk, st):
    c, ref = RH.ppo_get(pid, mk)
    RH.check_ppo_head(be, DEV, c, st, 'hip', ref)


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_ppo_head_scale_records(be, st):
    for pid, mk, _ in RH.ppo_plan():
        if pid in ('257x33-mgNone-random', '300x64-ls2-ec0.01'):
            c, ref = RH.ppo_get(pid, mk)
            RH.check_ppo_record(be, DEV, c, st, 'hip')
            if st == torch.float16:
                RH.check_ppo_saturation(be, DEV, c, 'hip', ref)


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_head_scale_records(be, st):
    RH.check_records(be, DEV, st, 'hip')


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_disc_head(be, st):
    for c in RH.disc_plan():
        RH.check_disc_head(be, DEV, c, st, 'hip')


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_enc_heads(be, st):
    for i, c in enumerate(RH.enc_plan()):
        RH.check_enc_head(be, DEV, c, st, 'hip', with_out=i % 2 == 0, with_db=i % 3 != 1)
        RH.check_enc_gp_seed(be, DEV, c, st, 'hip')
        RH.check_enc_gp_back(be, DEV, c, st, 'hip', with_db=i % 3 != 2)


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
@pytest.mark.parametrize('shape', RH.GP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gp_pieces(be, shape, st):
    for act in range(RH.ACT_RELU, RH.ACT_SOFTPLUS + 1):
        RH.check_gp(be, DEV, RH.gp_case(*shape, act, st), st, 'hip')


def test_reduce_sum(be):
    for n in (1, 255, 100003):
        for sq in (False, True):
            RH.check_reduce_sum(be, DEV, n, sq, 'hip')


@pytest.mark.parametrize('rows', RH.COLSUM_ROWS)
def test_colsum(be, rows):
    for cols in RH.COLSUM_COLS:
        RH.check_colsum(be, DEV, rows, cols, 'hip')


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_sqnorm(be, st):
    for rows, cols, pitch, col0 in RH.SQNORM_CASES:
        RH.check_sqnorm(be, DEV, rows, cols, pitch, col0, st, 'hip')


FIN_FLAGS = [(m, d, e, v) for m in (0, 1) for d in (0, 1) for e in (0, 1) for v in (0, 1)]


@pytest.mark.parametrize('masked,has_disc,has_enc,has_div', FIN_FLAGS)
def test_finalize_scalars(be, masked, has_disc, has_enc, has_div):
    """masked == 0 with has_div: RES_DIV_LOSS uses the denominator of ppo_head's diversity gradient, m_global.  The previous
    library divided by acc[MASK_SUM] (600 of m_global 1000 here: a factor 5 / 3)."""
    RH.check_finalize(be, DEV, RH.fin_acc(3, 1000), 1000, 333, masked, has_disc, has_enc, has_div, 'hip')


@pytest.mark.parametrize('kl,lr', [(0.05, 2e-5), (0.001, 2e-5), (0.01, 2e-5), (0.05, 1.2e-6), (0.001, 8e-3)])
def test_finalize_scalars_adaptive_rate(be, kl, lr):
    acc = RH.fin_acc(4, 1000)
    acc[RH.ACC['KL']] = kl * 1000
    RH.check_finalize(be, DEV, acc, 1000, 250, 1, 1, 1, 1, 'hip', lr=lr, kl_threshold=0.008)
