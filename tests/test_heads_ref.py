"""tests/ref_heads.py pinned without a GPU: the emulator (tests/emu_backend.py, tests/emu_learned_sigma.py) run over every
case of tests/test_gpu_heads.py and held to the same bounds - so cases, margins and bounds are satisfiable; eight single-term
wrong restatements of the reference, each of which must fail a bound on at least one case - so the bounds have teeth; and the
conditions of the fixtures: the margins to every branch threshold and the number of rows in every branch."""
import inspect

import pytest
import torch

from ase_amd import lib as L
from tests import ref_heads as RH
from tests.emu_learned_sigma import LearnedSigmaEmu

F32, F64 = RH.F32, RH.F64
ST_IDS = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}
PPO = [(pid, mk, st) for pid, mk, sts in RH.ppo_plan() for st in sts]


@pytest.fixture(scope='module')
def emu():
    return LearnedSigmaEmu()


def test_slot_numbers_are_the_library_s():
    assert all(getattr(L, 'ACC_' + k) == v for k, v in RH.ACC.items()) and RH.ACC_COUNT == L.ACC_COUNT
    assert all(getattr(L, 'RES_' + k) == v for k, v in RH.RES.items()) and RH.RES_COUNT == L.RES_COUNT
    assert (RH.LS_FROZEN, RH.LS_VECTOR, RH.LS_ROWS) == (L.LS_FROZEN, L.LS_VECTOR, L.LS_ROWS)
    assert [RH.ACT_RELU, RH.ACT_TANH, RH.ACT_SILU, RH.ACT_ELU, RH.ACT_GELU, RH.ACT_SIGMOID, RH.ACT_SELU, RH.ACT_SOFTPLUS] == \
        [L.ACT_RELU, L.ACT_TANH, L.ACT_SILU, L.ACT_ELU, L.ACT_GELU, L.ACT_SIGMOID, L.ACT_SELU, L.ACT_SOFTPLUS]


# ------------------------------------------------------------------------------------------------ the emulator on every case
@pytest.mark.parametrize('pid,mk,st', PPO, ids=[f'{p}-{ST_IDS[s]}' for p, _, s in PPO])
def test_emulator_ppo_head(emu, pid, mk, st):
    c, ref = RH.ppo_get(pid, mk)
    RH.check_ppo_head(emu, 'cpu', c, st, 'emu', ref)


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_emulator_ppo_records(emu, st):
    for pid, mk, _ in RH.ppo_plan():
        if pid in ('257x33-mgNone-random', '300x64-ls2-ec0.01'):
            c, ref = RH.ppo_get(pid, mk)
            RH.check_ppo_record(emu, 'cpu', c, st, 'emu')
            if st == torch.float16:
                RH.check_ppo_saturation(emu, 'cpu', c, 'emu', ref)


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_emulator_records(emu, st):
    RH.check_records(emu, 'cpu', st, 'emu')


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_emulator_disc_head(emu, st):
    for c in RH.disc_plan():
        RH.check_disc_head(emu, 'cpu', c, st, 'emu')


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_emulator_enc_heads(emu, st):
    for i, c in enumerate(RH.enc_plan()):
        RH.check_enc_head(emu, 'cpu', c, st, 'emu', with_out=i % 2 == 0, with_db=i % 3 != 1)
        RH.check_enc_gp_seed(emu, 'cpu', c, st, 'emu')
        RH.check_enc_gp_back(emu, 'cpu', c, st, 'emu', with_db=i % 3 != 2)


@pytest.mark.parametrize('st', RH.STORAGES, ids=ST_IDS.values())
def test_emulator_gp_pieces(emu, st):
    for rows, width, pitch in RH.GP_SHAPES[:3]:
        for act in range(RH.ACT_RELU, RH.ACT_SOFTPLUS + 1):
            RH.check_gp(emu, 'cpu', RH.gp_case(rows, width, pitch, act, st), st, 'emu')


def test_emulator_sums(emu):
    for n in (1, 255, 100003):
        for sq in (False, True):
            RH.check_reduce_sum(emu, 'cpu', n, sq, 'emu')
    for rows in RH.COLSUM_ROWS:
        for cols in RH.COLSUM_COLS:
            RH.check_colsum(emu, 'cpu', rows, cols, 'emu')
    for st in RH.STORAGES:
        for rows, cols, pitch, col0 in RH.SQNORM_CASES:
            RH.check_sqnorm(emu, 'cpu', rows, cols, pitch, col0, st, 'emu')


FIN_FLAGS = [(m, d, e, v) for m in (0, 1) for d in (0, 1) for e in (0, 1) for v in (0, 1)]


@pytest.mark.parametrize('masked,has_disc,has_enc,has_div', FIN_FLAGS)
def test_emulator_finalize_scalars(emu, masked, has_disc, has_enc, has_div):
    """has_div with masked == 0 is the case both the kernel and the emulator had wrong: RES_DIV_LOSS divided the sum by
    acc[MASK_SUM] where ase_hip_ppo_head's gradient divides by m_global."""
    RH.check_finalize(emu, 'cpu', RH.fin_acc(3, 1000), 1000, 333, masked, has_disc, has_enc, has_div, 'emu')


@pytest.mark.parametrize('kl,lr,expect', [(0.05, 2e-5, 2e-5 / 1.5), (0.001, 2e-5, 3e-5), (0.01, 2e-5, 2e-5), (0.05, 1.2e-6, 1e-6),
                                          (0.001, 8e-3, 1e-2)])
def test_emulator_adaptive_rate(emu, kl, lr, expect):
    acc = RH.fin_acc(4, 1000)
    acc[RH.ACC['KL']] = kl * 1000
    RH.check_finalize(emu, 'cpu', acc, 1000, 250, 1, 1, 1, 1, 'emu', lr=lr, kl_threshold=0.008)
    assert abs(RH.finalize(acc, 1000, 250, 1, 1, 1, 1, RH.FIN_CFG, lr, 0.008)[1] - expect) <= 1e-18


# ------------------------------------------------------------------------------------------------ the fixtures' conditions
def test_margins_and_branch_counts():
    seen = 0
    for pid, mk, _ in RH.ppo_plan():
        c, (r64, r32) = RH.ppo_get(pid, mk)
        if c['nan_row'] is not None:
            continue
        assert not RH.ppo_margins(c, r64).any(), pid                      # every row clear of every threshold, none left out
        if c['M'] >= 257:
            n = RH.ppo_branches(c, r64)
            assert all(v >= 8 for v in n.values()), (pid, n)
            seen += 1
        if c['div_on']:
            zd = 0.5 - 0.5 * (c['new_z'].double() * c['z'].double()).sum(-1)
            assert int((zd == 0).sum()) >= len(range(4, c['M'], 5)), pid           # new_z == z rows: z_diff exactly 0
        if c['ties']:
            assert float(c['adv'][0]) == 0 and float(c['value'][1]) == float(c['old_values'][1])
            assert float(c['value'][2] - c['old_values'][2]) == 0.25 and float(c['value'][3] - c['old_values'][3]) == -0.25
            assert bool((c['mu'][5, ::2] == 1).all()) and bool((c['mu'][6, ::2] == -1).all())
            # the clamp passes its gradient at the boundary, as torch.clamp does: the diversity gradient of those elements is
            # the ungated one (bound loss: zero there)
            assert bool((r64['d_mu'][5, ::2] != 0).all()) and bool((r64['d_mu'][c['M'] + 5, ::3] != 0)[c['mu'][5, ::3].abs() <= 1].all())
    assert seen >= 30
    for c in RH.disc_plan():
        assert bool(((c['logit'].abs() >= RH.MARGIN) | (c['logit'] == 0)).all())
        if c['amb'] >= 85:
            a, d = c['logit'][:2 * c['amb']], c['logit'][2 * c['amb']:]
            assert int((a == 0).sum()) >= 2 and int((d == 0).sum()) >= 2 and 100.0 in a and -100.0 in a and 100.0 in d and -100.0 in d


def test_policy_kl_rows_are_restated_policy_kl():
    from oracle import restated as R
    c = RH.ppo_case(257, 33, ls_mode=RH.LS_ROWS)
    out = RH.ppo_head(c)
    want = R.policy_kl(out['m'], torch.exp(c['logstd'].double()), c['old_mu'].double(), c['old_sigma'].double())
    assert abs(float(out['terms']['KL'].mean()) - float(want)) <= 1e-14


# ------------------------------------------------------------------------------------------------ the bounds have teeth
def _patched(fn, old, new):
    """A copy of a reference function with one term restated wrongly."""
    src = inspect.getsource(fn)
    assert src.count(old) == 1, (fn.__name__, old)
    ns = dict(vars(RH))
    exec(src.replace(old, new), ns)
    return ns[fn.__name__]


def _caught(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _ppo_wrong(old, new, cases, outputs=('d_mu', 'd_value'), sums=()):
    wrong = _patched(RH.ppo_head, old, new)
    hits = 0
    for c in cases:
        r64, r32, w = RH.ppo_head(c), RH.ppo_head(c, F32), wrong(c)
        hits += any(_caught(lambda k=k: RH.within(w[k], r64[k], r32[k], 'wrong ' + k)) for k in outputs)
        hits += any(_caught(lambda k=k: RH.sum_within(float(w['terms'][k].sum()), r64['terms'][k], r32['terms'][k], 'wrong ' + k))
                    for k in sums)
    return hits


def test_wrong_restatements_are_caught():
    masked = RH.ppo_case(257, 33, masked='random', Z=64, m_global=2 * 257 + 3)
    plain = RH.ppo_case(300, 64, Z=64)
    # the right restatement passes its own bound (the harness of this test is not what fails)
    r64, r32 = RH.ppo_head(masked), RH.ppo_head(masked, F32)
    RH.within(r32['d_mu'], r64['d_mu'], r32['d_mu'], 'f32 run d_mu')
    # 3. the critic term divided by the mask sum
    assert _ppo_wrong("cc * c_loss.sum() / c['m_global']", 'cc * c_loss.sum() / S', [masked], ('d_value',)) == 1
    # 4. the KL masked
    assert _ppo_wrong("'KL': kl,", "'KL': mk * kl,", [masked], (), ('KL',)) == 1
    # 5. the factor 2 of the bound-loss gradient dropped (the forward value kept)
    assert _ppo_wrong('bc * (mk * b_loss).sum() / S', '(bc * (mk * b_loss).sum() / S) * 0.5 + (bc * (mk * b_loss).sum() / S).detach() * 0.5',
                      [masked, plain], ('d_mu',)) == 2
    # 6. the diversity gradient not gated by |mu| <= 1 (the clamp's forward value kept)
    assert _ppo_wrong('torch.square(torch.clamp(m, -1.0, 1.0) - torch.clamp(m2, -1.0, 1.0))',
                      'torch.square((m + (torch.clamp(m, -1.0, 1.0) - m).detach()) - (m2 + (torch.clamp(m2, -1.0, 1.0) - m2).detach()))',
                      [masked, plain], ('d_mu',)) == 2
    # 1. the demo BCE divided by 2 amb; 2. amb where amb_global belongs
    c = RH.disc_case(86, 4 * 86, 1)
    d64, d32 = (RH.disc_head(c['logit'], 86, 4 * 86, 5.0, dt) for dt in (F64, F32))
    for old, new in (('td.sum() / amb_global', 'td.sum() / (2 * amb_global)'),
                     ('ta.sum() / (2 * amb_global) + td.sum() / amb_global', 'ta.sum() / (2 * amb) + td.sum() / amb')):
        w = _patched(RH.disc_head, old, new)(c['logit'], 86, 4 * 86, 5.0)
        assert _caught(lambda: RH.within(w['d_logit'], d64['d_logit'], d32['d_logit'], 'wrong d_logit'))
    # 7. the -3 a eh (eh . r) term of J with a 2; 8. the encoder gradient not projected (-z / n).  The analytic forms with the
    # right terms pass the same bounds.
    e = RH.enc_case(517, 64)
    ev, z, du = e['e'].double(), e['z'].double(), e['du'].double()
    n = ev.norm(dim=-1, keepdim=True)
    h = ev / n
    a, hr, zr = (h * z).sum(-1, keepdim=True), (h * du).sum(-1, keepdim=True), (z * du).sum(-1, keepdim=True)
    j64, j32 = RH.enc_gp(e['e'], e['z'], e['du']), RH.enc_gp(e['e'], e['z'], e['du'], F32)
    J = lambda k: (z * hr + h * zr + a * du - k * a * h * hr) / (n * n)
    RH.within(J(3.0), j64, j32, 'analytic J')
    assert _caught(lambda: RH.within(J(2.0), j64, j32, 'wrong J'))
    g64, g32 = (RH.enc_head(e['e'], e['z'], e['amb_global'], 5.0, dt)['d_e'] for dt in (F64, F32))
    sc = 5.0 / e['amb_global']
    RH.within(-sc * (z - h * a) / n, g64, g32, 'analytic d_e')
    assert _caught(lambda: RH.within(-sc * z / n, g64, g32, 'wrong d_e'))
