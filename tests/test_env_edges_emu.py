"""The edge fixture tests/golden/env_edges.pt (scripts/make_golden_env_edges.py) on the CPU: the conditions the generator
asserted, ``EmuEnvTensors`` and ``EmuEnvStep`` on every group under the bounds of the device tests (tests/env_edge_cases.py),
and thirteen restatements with ONE term wrong, each shown to fail at least one recorded case - the defects the suite could not
notice before: a ``>`` written as ``>=``, a wrong component, a mask on the wrong test, a clamp that drops a NaN."""
import math

import pytest
import torch

from tests import env_edge_cases as EC
from tests.emu_env_step import EmuEnvStep
from tests.emu_env_tensors import EmuEnvTensors


def _everything(be, stats=None):
    """Every group through the separate entries of `be` -> the stats; raises AssertionError at the first case that differs."""
    stats = EC.Stats() if stats is None else stats
    for name, grp in EC.groups('reset'):
        EC.run_reset_group(be, name, grp, 'cpu', stats)
    for name, grp in EC.groups('task'):
        for task in EC.TASKS:
            EC.run_task(be, name, grp, 'cpu', stats, task)
    for name, grp in EC.groups('obs'):
        EC.run_obs_group(be, name, grp, 'cpu', stats)
    return stats


# ---- the fixture's own conditions ---------------------------------------------------------------------------------------------
def test_fixture_holds_tensors_and_plain_lists_and_is_small():
    import os
    assert os.path.getsize(EC.GOLDEN) < 1 << 20

    def plain(x):
        if torch.is_tensor(x) or isinstance(x, (int, float, str, bool, type(None))):
            return True
        if isinstance(x, (list, tuple)):
            return all(plain(v) for v in x)
        return isinstance(x, dict) and all(plain(k) and plain(v) for k, v in x.items())
    assert plain(EC.load())


def test_every_branch_is_taken_and_not_taken():
    G = EC.load()
    for name, grp in EC.groups():
        if grp['n'] < 15 or grp['kind'] == 'obs':
            continue
        for k, m in zip(G['reset_masks' if grp['kind'] == 'reset' else 'task_masks'], grp['masks']):
            assert min(int(m.sum()), int((~m).sum())) >= 4, (name, k)


def test_truth_table_is_complete():
    keys = ('fall_contact', 'nonstrike_contact', 'fall_height', 'tar_has_contact', 'progress>1', 'progress>=max-1')
    seen = set()
    for name in ('reset_truth', 'reset_truth_short'):
        grp = EC.group(name)
        seen |= {tuple(bool(EC.mask(grp, k)[r]) for k in keys) for r in range(grp['n'])}
    assert len(seen) == 48 and all(fc or not nsc for fc, nsc, *_ in seen)
    assert EC.group('reset_truth')['split_rows'] >= 8


def test_non_planted_rows_keep_the_margin():
    m = EC.load()['margin']
    for name, grp in EC.groups():
        i, rows = grp['inputs'], grp['free_rows']
        if grp['kind'] == 'reset' and rows:
            c = i['contact_forces'][rows].abs().double()
            assert ((c - 0.1).abs() >= m).all() and ((c - 1.0).abs() >= m).all(), name
            assert ((i['body_pos'][rows][..., 2].double() - i['termination_heights'].double()).abs() >= m).all(), name
            assert ((i['tar_contact_forces'][rows][:, :2].abs().double() - 1.0).abs() >= m).all(), name
        if grp['kind'] == 'task':
            root, dt = i['root_states'][rows, 0:3].double(), grp['dt']
            vel = (root - i['prev_root_pos'][rows].double())[:, :2] / dt
            diff = i['tar_pos_loc'][rows].double() - root[:, :2]
            sdir = torch.nn.functional.normalize(i['tar_states'][rows, :2].double() - root[:, :2], dim=-1)
            q = i['tar_states'][rows, 3:7].double()
            for qty, thr in (((i['tar_dir'][rows].double() * vel).sum(-1), 0.0), ((diff * diff).sum(-1), 0.5),
                             ((torch.nn.functional.normalize(diff, dim=-1) * vel).sum(-1), 0.0), ((sdir * vel).sum(-1), 0.0),
                             ((2.0 * q[:, 3] ** 2 - 1.0) + 2.0 * q[:, 2] * q[:, 2], 0.2)):
                assert ((qty - thr).abs() >= m).all(), name


def test_runs_agree_outside_the_tie_rows_and_share_their_nan_pattern():
    for name, grp in EC.groups():
        rest = [r for r in range(grp['n']) if r not in grp['tie_rows']]
        if grp['kind'] == 'reset':
            assert torch.equal(grp['f32'][..., rest], grp['f64'][..., rest]), name
            assert all(w.startswith('tie') for r, w in grp['planted'] if r in grp['tie_rows'])
        elif grp['kind'] == 'task':
            for f in grp['f32']:
                a, b = grp['f32'][f], grp['f64'][f]
                assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b)), (name, f)
            # outside the tie rows the strike reward is 1 in both runs or in neither
            a, b = grp['f32']['strike_rew'][rest], grp['f64']['strike_rew'][rest]
            assert torch.equal(a == 1.0, b == 1.0)
            assert any(torch.isnan(grp['f32'][f]).any() for f in grp['f32'])
        else:
            for k in EC.FLAGS:
                a, b = EC.obs_want(grp, 'f32', *k), EC.obs_want(grp, 'f64', *k)
                assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b)), name


def test_wide_allowances_are_named_and_few():
    G = EC.load()
    total = wide = 0
    for name, grp in EC.groups():
        count = 0
        if grp['kind'] == 'obs':
            count = grp['f64']['obs_max'].numel() + 3 * grp['n'] * 7
        elif grp['kind'] == 'task':
            count = sum(v.numel() for v in grp['f64'].values())
        over = any(EC.allowance(grp, f) > G['wide_bar'] for f in grp['e_ref'])
        assert over == grp['wide'] and (not over or name in ('obs_ill_conditioned', 'obs_large')), name
        total += count
        wide += count if over else 0
    assert total == G['float_elements'] and wide == G['wide_elements'] and wide <= G['wide_share'] * total


# ---- the stand-ins on every group -----------------------------------------------------------------------------------------------
def test_emulator_matches_the_recording_on_every_group():
    stats = _everything(EmuEnvTensors())
    assert sum(s['guard_words'] for s in stats.values()) > 10000
    assert sum(s['tie_elements'] for s in stats.values()) >= 3


@pytest.mark.parametrize('name', EC.names())
def test_emulated_post_step_on_every_group(name):
    grp, be, stats = EC.group(name), EmuEnvStep(), EC.Stats()
    for task in EC.post_step_tasks(grp):
        EC.run_post_step(be, name, grp, 'cpu', stats, task, 0, math.inf, False)
        EC.run_post_step(be, name, grp, 'cpu', stats, task, 1, 5.0, True, local_root=False)


# ---- thirteen restatements with one term wrong: each fails at least one case --------------------------------------------------
def _drop_nan(x):
    """fmaxf(x, 0): a NaN becomes 0 - what the kernel's clamps did before they were floor_nan."""
    return torch.where(torch.isnan(x), torch.zeros_like(x), x.clamp_min(0.0))


class _IgnoresLocalRoot(EmuEnvTensors):
    def humanoid_obs_max(self, body_pos, body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs, obs, col_offset=0, env_ids=None):
        super().humanoid_obs_max(body_pos, body_rot, body_vel, body_ang_vel, False, root_height_obs, obs, col_offset, env_ids)


WRONG = {
    'contact >=': dict(_loud=staticmethod(lambda f, t: f >= t)),
    'height <=': dict(_low=staticmethod(lambda h, t: h <= t)),
    'progress >= 1': dict(_started=staticmethod(lambda p: p >= 1)),
    'timeout >': dict(_timed_out=staticmethod(lambda p, m: p > m - 1)),
    "the target's z counted": dict(_tar_cols=3),
    'the height test not masked by the contact bodies': dict(_mask_height=False),
    'strike bodies excluded from fall_contact': dict(_strike_falls=False),
    'the contact maximum over x and y only': dict(_force_cols=2),
    'a clamp that drops NaN': dict(_clamp0=staticmethod(_drop_nan)),
    'speed < 0': dict(_stopped=staticmethod(lambda s: s < 0)),
    'pos_err <= 0.5': dict(_near=staticmethod(lambda e: e <= 0.5)),
    'rot_err <= 0.2': dict(_upright=staticmethod(lambda e: e <= 0.2)),
    'local_root_obs ignored': None,
}


@pytest.mark.parametrize('wrong', list(WRONG))
def test_a_wrong_restatement_fails(wrong):
    cls = _IgnoresLocalRoot if WRONG[wrong] is None else type('Wrong', (EmuEnvTensors,), WRONG[wrong])
    with pytest.raises(AssertionError) as e:
        _everything(cls())
    print(f'{wrong}: {str(e.value)[:300]}')


def test_the_nan_dropping_clamp_fails_where_the_issue_predicts():
    """The kernel's former fmaxf clamps, restated: the strike reward with a NaN target rotation, the heading reward with a NaN
    tar_face_dir and the location / strike reward with a NaN prev_root_pos come out finite where the reference has NaN."""
    grp = EC.group('tasks')
    be = type('Wrong', (EmuEnvTensors,), WRONG['a clamp that drops NaN'])()
    i = EC.full_state(grp)
    rows = {w: r for r, w in grp['planted']}
    for task, what in (('strike', 'non-finite: NaN target rotation w'), ('heading', 'non-finite: NaN tar_face_dir y'),
                       ('location', 'non-finite: NaN previous root position x'), ('strike', 'non-finite: NaN previous root position y')):
        r = rows[what]
        rew = torch.zeros(grp['n'])
        be.task_reward(EC.KIND[task], rew, **EC.task_operands(grp, i, task, 'rew'))
        assert math.isnan(float(grp['f32'][f'{task}_rew'][r])) and math.isfinite(float(rew[r])), (task, what)
