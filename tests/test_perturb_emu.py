"""The projectile launches of the perturbation task without a GPU: the stand-in tests/emu_perturb.py against
the recording tests/golden/perturb.pt of the reference's unmodified ``HumanoidPerturb._update_proj``, the schedule and the draw
table of tests/ref_perturb.py, ``ProjectileLauncher.draw``, the host checks of ``ase_hip_proj_launch`` and
``HumanoidEnv(perturb=...)`` on the emulator."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ase_amd import lib as L
from ase_amd.humanoid_env import HumanoidEnv
from ase_amd.perturb import PERTURB_OBJS, ProjectileLauncher
from tests import emu_perturb as E
from tests import env_step_cases as CS
from tests import ref_perturb as RP
from tests import ref_rollout as RR


@pytest.fixture(scope='module')
def G():
    return E.load_fixture()


@pytest.fixture(scope='module')
def fx():
    return CS.load()


def _due(case):
    return [st for st in case['chain'] if st['slot'] >= 0]


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_fixture_conditions(G):
    assert os.path.getsize(os.path.join(E.GOLDEN, 'perturb.pt')) < 64 * 1024
    assert G['num_envs'] == 32 and tuple(G['steps']) == PERTURB_OBJS == RP.PERTURB_STEPS
    assert G['timesteps'] == [60, 67, 77, 112, 114, 116, 119, 121, 123, 126, 128, 188, 488] == RP.PERTURB_TIMESTEPS.tolist()
    assert sorted(c['actors'] for c in G['cases'].values()) == [14, 15] and G['tar_body'] == 1
    for case in G['cases'].values():
        assert [st['progress'] for st in case['chain']] == [59, 60, 77, 488, 489 + 67]
        assert [st['slot'] for st in case['chain']] == [-1, 0, 2, 12, 1]
        assert case['after'].shape == (32 * case['actors'], 13) and case['after'].dtype == torch.float32
        _, proj = E.views(G, case['after'], case['actors'])
        for st in _due(case):
            u, eps = RP.split(st['draws'])
            assert u.dtype == torch.float32 and bool(((u > 0) & (u < 1)).all()) and bool(torch.isfinite(eps).all())
            row = proj[:, st['slot']]
            for g, cols in E.GROUPS.items():          # the cap of the generator: a bad draw cannot loosen the device tests
                assert 0 < st['e_ref'][g] <= G['roundings'] * 2.0 ** -24 * float(row[:, cols].abs().max()), (st['progress'], g)


def test_stand_in_is_bitwise_the_recording_in_f32_and_within_e_ref_in_f64(G):
    for name, case in G['cases'].items():
        A = case['actors']
        f32, f64 = E.replay(G, case, torch.float32), E.replay(G, case, torch.float64)
        assert torch.equal(f32, case['after']), name
        before = E.packed_before(G, A)
        _, proj = E.views(G, case['after'], A)
        _, proj64 = E.views(G, f64, A)
        _, proj0 = E.views(G, before, A)
        written = [st['slot'] for st in _due(case)]
        others = [k for k in range(13) if k not in written]
        # untouched slots and actors are part of the record
        assert torch.equal(proj[:, others], proj0[:, others]) and torch.equal(proj64[:, others], proj0[:, others].double())
        assert torch.equal(case['after'].view(32, A, 13)[:, :A - 13], before.view(32, A, 13)[:, :A - 13])
        for st in _due(case):
            row, row64 = proj[:, st['slot']], proj64[:, st['slot']]
            assert torch.equal(row[:, E.CONSTANT_COLS], E.CONSTANT.expand(32, 7))
            assert torch.equal(row64[:, E.CONSTANT_COLS], E.CONSTANT.double().expand(32, 7))
            for g, cols in E.GROUPS.items():
                err = float((row[:, cols].double() - row64[:, cols]).abs().max())
                assert err == st['e_ref'][g], (name, st['progress'], g, err, st['e_ref'][g])
            assert not torch.equal(row, proj0[:, st['slot']])


def test_not_due_writes_nothing_and_reports_it(G):
    case = G['cases']['A14']
    packed = E.packed_before(G, 14)
    root, proj = E.views(G, packed, 14)
    slot, ids, draws = torch.full((1,), 7, dtype=torch.int32), torch.full((32,), 7, dtype=torch.int32), torch.full((32, 7), 7.0)
    rng = torch.tensor([5, 11], dtype=torch.int64)
    E.EmuProjLaunch().proj_launch(root, G['body_pos'], G['body_vel'], proj, progress_buf=torch.full((32,), 59, dtype=torch.int64),
                                  timesteps=E.timesteps_of(G), rng_state=rng, slot_out=slot, ids_out=ids, draws_out=draws)
    assert torch.equal(packed, E.packed_before(G, 14)) and int(slot) == -1 and bool((ids == -1).all()) and bool((draws == 7.0).all())
    assert rng.tolist() == [5, 12]                       # a call is one stream position, due or not
    assert case['chain'][0]['slot'] == -1


# ---- the launcher ---------------------------------------------------------------------------------------------------------------
def test_draw_equals_the_recorded_draws_in_call_order(G):
    la = ProjectileLauncher(E.EmuProjLaunch(), 32)
    for case in G['cases'].values():
        for st in _due(case):
            torch.manual_seed(st['seed'])
            plan = la.draw(32)
            u, eps = RP.split(st['draws'])
            assert torch.equal(plan['u'], u) and torch.equal(plan['eps'], eps), st['seed']
    g = torch.Generator().manual_seed(3)
    torch.manual_seed(3)
    want = la.draw(5)
    got = ProjectileLauncher(E.EmuProjLaunch(), 32, generator=g).draw(5)
    assert torch.equal(got['u'], want['u']) and torch.equal(got['eps'], want['eps'])


def test_launcher_apply_is_the_recording_and_update_follows_environment_zero(G):
    case = G['cases']['A15']
    la = ProjectileLauncher(E.EmuProjLaunch(), 32, seed=9)
    assert la.perturb_timesteps == tuple(G['timesteps']) and la.timesteps.tolist() == G['timesteps'] and la.timesteps.dtype == torch.int32
    assert la.params == G['params'] and la.tar_body == 1 and la.rng_state.tolist() == [9, 0]
    packed = E.packed_before(G, 15)
    root, proj = E.views(G, packed, 15)
    state = dict(humanoid_root_states=root, rigid_body_pos=G['body_pos'], rigid_body_vel=G['body_vel'], proj_states=proj)
    for st in _due(case):
        u, eps = RP.split(st['draws'])
        la.apply(state, {'u': u, 'eps': eps}, st['slot'])
        assert int(la.slot_word) == st['slot'] and la.launch_ids.tolist() == list(range(32))
    assert torch.equal(packed, case['after']) and la.rng_state.tolist() == [9, 0]
    # update: environment 0 due, every other row not -> all launch; the converse -> none does
    progress = torch.full((32,), 59, dtype=torch.int64)
    progress[0] = 67
    before = packed.clone()
    la.update(state, progress)
    assert int(la.slot_word) == 1 and la.launch_ids.tolist() == list(range(32)) and la.rng_state.tolist() == [9, 1]
    changed = (packed.view(32, 15, 13) != before.view(32, 15, 13)).any(-1)
    assert bool(changed[:, 3].all()) and int(changed.sum()) == 32
    d = RP.device_draws(range(32), 9, 0)
    twin = before.clone()
    r2, p2 = E.views(G, twin, 15)
    u, eps = RP.split(d)
    E.EmuProjLaunch().proj_launch(r2, G['body_pos'], G['body_vel'], p2, slot=1, u=u, eps=eps)
    assert torch.equal(twin, packed)
    progress[:] = 67
    progress[0] = 59
    before = packed.clone()
    la.update(state, progress)
    assert int(la.slot_word) == -1 and bool((la.launch_ids == -1).all()) and torch.equal(packed, before) and la.rng_state.tolist() == [9, 2]
    # explicit launch of a list with ids outside the range: those rows only, one stream position
    la.launch(state, 5, env_ids=[3, -1, 40, 7])
    changed = (packed.view(32, 15, 13) != before.view(32, 15, 13)).any(-1)
    assert changed.nonzero().tolist() == [[3, 7], [7, 7]] and la.rng_state.tolist() == [9, 3] and int(la.slot_word) == 5
    assert bool((la.launch_ids == -1).all())              # a call on an id list writes the word, not the full-length list


def test_launcher_refusals():
    be = E.EmuProjLaunch()
    with pytest.raises(ValueError, match='positive'):
        ProjectileLauncher(be, 4, objs=(3, 0, 2))
    with pytest.raises(ValueError, match='projectiles'):
        ProjectileLauncher(be, 4, objs=())
    with pytest.raises(ValueError, match='projectiles'):
        ProjectileLauncher(be, 4, objs=[1] * 33)
    la = ProjectileLauncher(be, 4, objs=(3, 2))
    z = torch.zeros
    ok = dict(humanoid_root_states=z(4, 13), rigid_body_pos=z(4, 2, 3), rigid_body_vel=z(4, 2, 3), proj_states=z(4, 2, 13))
    for bad in (z(4, 1, 13), z(3, 2, 13), z(4, 2, 12), z(4, 2, 26)[:, :, ::2]):
        with pytest.raises(ValueError, match='proj_states'):
            la.update(dict(ok, proj_states=bad), z(4, dtype=torch.int64))
    with pytest.raises(ValueError, match='rigid_body_pos'):
        la.update(dict(ok, rigid_body_pos=z(4, 2, 6)[:, :, ::2]), z(4, dtype=torch.int64))


# ---- the schedule and the draw table --------------------------------------------------------------------------------------------
def test_schedule_is_the_reference_for_every_counter_value():
    perturb_timesteps = np.cumsum([60, 7, 10, 35, 2, 2, 3, 2, 2, 3, 2, 60, 300])
    be = E.EmuProjLaunch()
    packed = torch.zeros(2 * 14, 13)
    v = packed.view(2, 14, 13)
    slot, ids = torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    ts = torch.tensor(perturb_timesteps.tolist(), dtype=torch.int32)
    hits = 0
    for t in range(1001):
        where = np.where(perturb_timesteps == t % (perturb_timesteps[-1] + 1))[0]
        want = int(where[0]) if len(where) > 0 else -1
        assert RP.due_slot(t) == want, t
        be.proj_launch(v[:, 0], torch.zeros(2, 2, 3), torch.zeros(2, 2, 3), v[:, 1:], progress_buf=torch.tensor([t, 60]), timesteps=ts,
                       u=torch.full((2, 4), 0.5), eps=torch.zeros(2, 3), slot_out=slot, ids_out=ids)
        assert int(slot) == want and ids.tolist() == ([0, 1] if want >= 0 else [-1, -1]), t
        hits += want >= 0
    assert hits == 26                                     # every object once in 0 .. 488 and once more in 489 .. 1000


def test_device_draw_table_element_by_element():
    seed, offset = (1 << 33) + 12345, (1 << 32) + 7
    envs = [0, 1, 63, 64, 129, (1 << 29) + 3]
    d = RP.device_draws(envs, seed, offset)
    d64 = RP.device_draws(envs, seed, offset, torch.float64)
    assert d.shape == (len(envs), 7) and d.dtype == torch.float32
    for i, e in enumerate(envs):
        for j in range(7):
            w = RR.philox4x32_10(8 * e + j, offset, seed)
            if j in (0, 1, 2, 6):
                want = float(np.float32(int(w[2][0]) >> 8) * np.float32(2.0 ** -24))
                assert float(d[i, j]) == want == float(d64[i, j]) and 0.0 <= want < 1.0, (e, j)
            else:
                assert float(d[i, j]) == float(RR._box_muller(w[0], w[1], np.float32)[0]), (e, j)
                assert float(d64[i, j]) == float(RR._box_muller(w[0], w[1], np.float64)[0]), (e, j)
    u, eps = RP.split(d)
    assert torch.equal(u, d[:, [0, 1, 2, 6]]) and torch.equal(eps, d[:, 3:6]) and torch.equal(RP.join(u, eps), d)
    # another stream position, another environment: other draws
    assert not torch.equal(RP.device_draws(envs, seed, offset + 1), d) and not torch.equal(d[0], d[1])


# ---- single-term wrong restatements each miss a bound ----------------------------------------------------------------------------
class _Wrong(E.EmuProjLaunch):
    def __init__(self, wrong):
        self.wrong = wrong


def _misses(G, case, backend):
    """Which checks a stand-in misses on a case: 'bitwise' (f32 against the recording) and the groups beyond e_ref in f64."""
    out = set()
    if not torch.equal(E.replay(G, case, torch.float32, backend), case['after']):
        out.add('bitwise')
    _, got = E.views(G, E.replay(G, case, torch.float64, backend), case['actors'])
    _, ref = E.views(G, case['after'], case['actors'])
    for st in _due(case):
        for g, cols in E.GROUPS.items():
            if float((ref[:, st['slot'], cols].double() - got[:, st['slot'], cols]).abs().max()) > st['e_ref'][g]:
                out.add(g)
    return out


def test_wrong_restatements_miss_a_bound(G):
    case = G['cases']['A14']
    assert _misses(G, case, E.EmuProjLaunch()) == set()
    assert {'bitwise', 'position', 'velocity'} <= _misses(G, case, _Wrong('+d sin'))
    assert _misses(G, case, _Wrong('noise first')) == {'bitwise'}          # the same sum in another order: only the f32 bits show it
    assert _misses(G, case, _Wrong('velocity z')) == {'bitwise', 'velocity'}
    # the schedule from every environment's own counter: with environment 0 due and the others not, only row 0 is written
    progress = torch.full((32,), 59, dtype=torch.int64)
    progress[0] = 60
    u, eps = RP.split(case['chain'][1]['draws'])
    outs = []
    for be in (E.EmuProjLaunch(), _Wrong('own counter')):
        packed = E.packed_before(G, 14)
        root, proj = E.views(G, packed, 14)
        be.proj_launch(root, G['body_pos'], G['body_vel'], proj, progress_buf=progress, timesteps=E.timesteps_of(G), u=u, eps=eps)
        outs.append(proj[:, 0].clone())
    _, ref = E.views(G, case['after'], 14)
    assert torch.equal(outs[0], ref[:, 0]) and torch.equal(outs[1][0], ref[0, 0]) and not torch.equal(outs[1][1:], ref[1:, 0])


# ---- the host checks of the C entry: every refusal, without a launch -------------------------------------------------------------
LAST = b'body_pos / body_vel strides'        # the message of the entry's last check


def _entry_args(**kw):
    """Arguments that pass every check of the entry BUT THE LAST: vel_sb = 2 is below a body's three floats, so no call built
    here can reach the launch, whatever else it carries and whichever earlier check it is meant to show."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(progress_buf=p, timesteps=p, n_slots=13, slot=-1, env_ids=None, n_ids=0, u=None, eps=None, rng_state=p, advance=1,
             root_states=p, ld_root=13, body_pos=p, pos_se=6, pos_sb=3, body_vel=p, vel_se=6, vel_sb=2, n_bodies=2, tar_body=1,
             proj_states=p, ld_env=14 * 13, ld_slot=13, dist_min=4.0, dist_max=5.0, h_min=0.25, h_max=2.0, speed_min=30.0,
             speed_max=40.0, noise=0.1, slot_out=p, ids_out=p, draws_out=None, n_envs=4, stream=None)
    assert set(kw) <= set(a) and kw.get('vel_sb', 2) < 3, 'every call keeps the defect that the last check refuses'
    a.update(kw)
    return list(a.values()), buf, p


def _refusal(lib, **kw):
    args, keep, _ = _entry_args(**kw)
    rc = lib.ase_hip_proj_launch(*args)
    msg = lib.ase_hip_last_error()
    assert rc == -1 and msg.startswith(b'proj_launch:'), (kw, rc, msg)
    return msg


def test_every_refusal_of_the_entry_without_a_launch():
    """Every call carries vel_sb = 2, which the last check refuses, so nothing is ever launched - also not by a library whose
    earlier check was dropped or weakened.  A defect of an earlier check is shown by that check's own message; `passes` shows the
    good side: a value at the edge of a check gets past it and every other one, down to the last message."""
    lib = L.load()
    _, _, p = _entry_args()
    explicit = dict(slot=2, progress_buf=None, timesteps=None)
    defects = [
        (dict(n_envs=0), b'bad size'),
        (dict(n_envs=-4), b'bad size'),
        (dict(n_slots=0), b'n_slots 0 outside'),
        (dict(n_slots=33), b'n_slots 33 outside'),
        (dict(root_states=None), b'needs root_states'),
        (dict(body_pos=None), b'needs root_states'),
        (dict(body_vel=None), b'needs root_states'),
        (dict(proj_states=None), b'needs root_states'),
        (dict(slot=13), b'slot 13 outside'),
        (dict(slot=-2), b'slot -2 outside'),
        (dict(progress_buf=None), b'come with due mode'),
        (dict(timesteps=None), b'come with due mode'),
        (dict(slot=2), b'come with due mode'),
        (dict(explicit, timesteps=p), b'come with due mode'),
        (dict(explicit, n_ids=3), b'n_ids 3 without env_ids'),
        (dict(explicit, env_ids=p, n_ids=-1, ids_out=None), b'n_ids -1 with env_ids'),
        (dict(env_ids=p, n_ids=2, ids_out=None), b'due mode launches for every environment'),
        (dict(explicit, env_ids=p, n_ids=2), b'ids_out is the export'),
        (dict(u=p, eps=p), b'exactly one draw source, u or rng_state (both given)'),
        (dict(rng_state=None), b'exactly one draw source, u or rng_state (none given)'),
        (dict(eps=p), b'eps comes with u'),
        (dict(u=p, rng_state=None), b'eps comes with u'),
        (dict(ld_root=12), b'root_states row stride 12 below 13'),
        (dict(ld_root=-13), b'root_states row stride -13 below 13'),
        (dict(ld_env=12), b'proj_states strides'),
        (dict(ld_slot=12), b'proj_states strides'),
        (dict(ld_slot=0), b'proj_states strides'),
        (dict(n_bodies=0), b'tar_body 1 outside the 0 bodies'),
        (dict(tar_body=2), b'tar_body 2 outside the 2 bodies'),
        (dict(tar_body=-1), b'tar_body -1 outside'),
    ]
    for kw, text in defects:
        msg = _refusal(lib, **kw)
        assert text in msg and LAST not in msg, (kw, msg)

    def passes(**kw):
        msg = _refusal(lib, **kw)
        assert LAST in msg, (kw, msg)
    # the good side of every check: the values at its edge, and each mode's operand pattern, reach the last check
    passes()
    passes(n_envs=1)
    passes(n_slots=1, slot=-1)
    passes(n_slots=32)
    passes(n_slots=32, **dict(explicit, slot=31))
    passes(**dict(explicit, slot=0))
    passes(**dict(explicit, slot=12))
    passes(**dict(explicit, env_ids=p, n_ids=0, ids_out=None))
    passes(**dict(explicit, env_ids=p, n_ids=3, ids_out=None))
    passes(u=p, eps=p, rng_state=None)
    passes(advance=0, slot_out=None, ids_out=None, draws_out=p)
    passes(ld_root=13, ld_env=13, ld_slot=13)
    passes(ld_root=1 << 40, ld_env=1 << 40, ld_slot=1 << 36)
    passes(n_bodies=1, tar_body=0)
    passes(n_bodies=64, tar_body=63)
    # the last check's own cases, the other three strides varied beside the one every call carries; then that one alone
    for kw in (dict(pos_se=2), dict(vel_se=0), dict(pos_sb=2), dict(pos_se=-6, vel_se=2, pos_sb=-3), dict(vel_sb=-3),
               dict(pos_se=3, vel_se=3, pos_sb=3), dict(pos_se=1 << 40, vel_se=1 << 40, pos_sb=1 << 36)):
        passes(**kw)
    assert L.ABI_VERSION == 9 and lib.ase_hip_abi_version() == 9 and len(L.SIGNATURES['ase_hip_proj_launch']) == 35


# ---- HumanoidEnv(perturb=...) on the emulator -----------------------------------------------------------------------------------
class _NoEntry(E.EmuEnvPerturb):
    def proj_launch(self, *a, **kw):
        raise AssertionError('the default environment touches proj_launch')


def _raiser(what):
    def f(*a, **kw):
        raise AssertionError(f'{what} inside step')
    return f


def test_env_launches_on_the_schedule_of_environment_zero(fx, monkeypatch):
    Genv, clips, _ = fx
    env = E.make_env(E.EmuEnvPerturb(), 'cpu', Genv, clips, True, n=20)
    n, ph = env.num_envs, env.physics
    assert n == 20 and ph.state['proj_states'].shape == (n, 13, 13) and not ph.state['proj_states'].is_contiguous()
    env.reset()
    assert len(ph.pushed_projectiles) == 1 and ph.pushed_projectiles[0][1] is None and ph.pushed_projectiles[0][0].tolist() == list(range(n))
    env.progress_buf.copy_(54 + torch.arange(n) % 7)            # environment 0 reaches 60 at the seventh step; others before it
    parked = ph.state['proj_states'].clone()
    slots, recs = [], []
    for k in range(12):
        before = ph.state['proj_states'].clone()
        progress = env.progress_buf.clone()
        calls = len(ph.pushed_projectiles)
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, 'cpu', _raiser('Tensor.cpu'))
            m.setattr(torch.Tensor, 'nonzero', _raiser('Tensor.nonzero'))
            m.setattr(torch, 'rand', _raiser('torch.rand'))
            obs, rew, dones, infos = env.step(CS.actions_of(k, n, 31))
        after = ph.state['proj_states']
        slot = int(env.launcher.slot_word)
        slots.append(slot)
        assert slot == RP.due_slot(int(progress[0])) and env.launcher.rng_state.tolist() == [3 + 3, k + 1]
        # push_projectiles got the launcher's id list and word, once, before the counters moved on
        assert len(ph.pushed_projectiles) == calls + 1
        ids, word = ph.pushed_projectiles[-1]
        assert ids is env.launcher.launch_ids and word is env.launcher.slot_word
        changed = (after != before).any(-1)
        if slot >= 0:
            assert ids.tolist() == list(range(n)) and bool(changed[:, slot].all()) and int(changed.sum()) == n
            assert torch.equal(after[:, slot, E.CONSTANT_COLS], E.CONSTANT.expand(n, 7))
        else:
            assert bool((ids == -1).all()) and not bool(changed.any())
        # timeout only: terminate stays 0, a row resets when its counter reaches episodeLength - 1
        assert torch.equal(env.progress_buf, progress + 1) and not bool(infos['terminate'].any())
        assert torch.equal(dones != 0, env.progress_buf >= 63)
        done = dones.clone()                                   # (dones is reset_buf itself: the reset clears it)
        recs.append(done)
        env.reset_done(dones)
        assert ph.pushed_projectiles[-1][1] is None and torch.equal(ph.pushed_projectiles[-1][0] >= 0, done != 0)
    assert slots == [-1] * 6 + [0] + [-1] * 5                 # rows whose own counter passed 60 earlier launched nothing
    assert sum(int(d.sum()) for d in recs) >= n // 2 and torch.equal(ph.state['proj_states'][:, 1:], parked[:, 1:])
    # playback does not overwrite what the launch wrote
    assert not torch.equal(ph.state['proj_states'][:, 0], parked[:, 0])


def test_env_fused_and_unfused_steps_agree_on_the_emulator(fx):
    Genv, clips, _ = fx
    runs = [E.run_env(E.make_env(E.EmuEnvPerturb(), 'cpu', Genv, clips, fused, n=20), 12) for fused in (True, False)]
    for k, (a, b) in enumerate(zip(*runs)):
        for key in a:
            x, y = a[key], b[key]
            same = torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0)) if x.dtype.is_floating_point else torch.equal(x, y)
            assert same, (k, key)
    assert [int(r['slot']) for r in runs[0]] == [-1] * 6 + [0] + [-1] * 5


def test_default_environment_never_touches_the_entry(fx):
    Genv, clips, A = fx
    env = CS.make_env(_NoEntry(), 'cpu', Genv, clips, A, None, False, True)
    assert env.launcher is None and 'proj_states' not in env.physics.state and not hasattr(env.physics, 'pushed_projectiles')
    twin =CS.make_env(E.EmuEnvPerturb(), 'cpu', Genv, clips, A, None, False, True)
    a, b = CS.run(env, 3, True), CS.run(twin, 3, True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x['dones'], y['dones']) for x, y in zip(a[1], b[1]))
    with pytest.raises(AssertionError, match='without projectiles'):
        env.physics.push_projectiles(None, None)


def test_perturb_dict_reaches_the_launcher(fx):
    Genv, clips, _ = fx
    env = E.make_env(E.EmuEnvPerturb(), 'cpu', Genv, clips, True, perturb=dict(objs=(3, 2, 4), seed=77, speed_min=1.0, tar_body=4), K=4, n=8,
                     extra_actor=True)
    la = env.launcher
    assert la.perturb_timesteps == (3, 5, 9) and la.rng_state.tolist() == [77, 0] and la.params['speed_min'] == 1.0 and la.tar_body == 4
    assert env.physics.state['proj_states'].shape == (8, 4, 13) and 'target_states' in env.physics.state
    env.reset()
    env.progress_buf.fill_(2)
    seen = []
    for k in range(9):
        env.step(CS.actions_of(k, 8, 31))
        seen.append(int(la.slot_word))
    assert seen == [-1, 0, -1, 1, -1, -1, -1, 2, -1]


def test_constructor_refusals(fx):
    Genv, clips, A = fx
    be = E.EmuEnvPerturb()
    env = E.make_env(be, 'cpu', Genv, clips, True, n=8)
    cfg = CS.env_cfg(Genv, None, False)
    cfg['numEnvs'] = 8
    with pytest.raises(ValueError, match='no task and no get-up'):
        E.make_env(be, 'cpu', Genv, clips, True, n=8, task='heading')
    with pytest.raises(ValueError, match='no task and no get-up'):
        E.make_env(be, 'cpu', Genv, clips, True, n=8, getup=True)
    with pytest.raises(ValueError, match='needs a motion_lib'):
        E.make_env(be, 'cpu', Genv, clips, True, n=8, motion_lib=None)
    with pytest.raises(ValueError, match='None, True or a dict'):
        E.make_env(be, 'cpu', Genv, clips, True, n=8, perturb=False)
    with pytest.raises(ValueError, match='proj_states'):          # fewer projectiles than the schedule has objects
        E.make_env(be, 'cpu', Genv, clips, True, n=8, K=12)
    plain = CS.make_env(be, 'cpu', Genv, clips, A, None, False, True)
    with pytest.raises(ValueError, match='proj_states'):          # a physics without projectiles
        HumanoidEnv(be, plain.physics, CS.env_cfg(Genv, None, False), motion_lib=object(), perturb=True)
    ph = env.physics
    ph.push_projectiles = None
    with pytest.raises(ValueError, match='push_projectiles'):
        HumanoidEnv(be, ph, cfg, motion_lib=object(), perturb=True)
