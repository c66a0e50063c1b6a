"""The view-motion task on the MI355X: ``ase_hip_motion_sync`` through ``HipBackend``,
``torch.ops.ase_hip.motion_sync`` and ``ViewMotionEnv`` on ``ClipPhysics`` against tests/golden/view_motion.pt, the sampler
entry ``ase_hip_motion_state`` and the f64 restatement tests/ref_view_motion.py.

Every output is a window of a NaN-filled allocation with wider pitches (the humanoid's row beside NaN actors, the interleaved
dof state, bodies with pad columns); every sentinel is checked after each launch.  SYNC is bitwise ``motion_state`` at the same
(ids, t) for root, dof positions and body positions; zeros are +0.0 bit for bit; body rotations and the recorded cases are held
to 2 e_ref + 2^-23 max |ref| + 1e-7 against f64, e_ref = what the reference's own f32 run loses (recorded, or the f32
statement's own loss where the shape is beyond the recording).  The integer outputs are exact.
ASE_VIEW_MOTION_REPORT=<file> writes the case and element counts and the observed maxima (COVERAGE.md N17)."""
import json
import os

import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd import lib as L
from tests import emu_view_motion as E
from tests import ref_amp_obs as R
from tests import ref_view_motion as RV

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I64 = lambda x: torch.tensor(x, dtype=torch.int64)
REPORT = {'cases': 0, 'elements': 0, 'max_err_over_allowed': {}}


@pytest.fixture(scope='module')
def G():
    return RV.load_fixture()


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    yield HipBackend(DEV)
    path = os.environ.get('ASE_VIEW_MOTION_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(REPORT) + '\n')


def _dev(clips):
    out = {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in clips.items()}
    out['num_frames'], out['length_starts'] = out['num_frames'].to(torch.int32), out['length_starts'].to(torch.int32)
    return out


def _within(name, got, ref64, e_ref):
    bar = RV.allowance(e_ref, ref64)
    err = float((got.double().cpu() - ref64).abs().nan_to_num(nan=1e9).max())
    print(f'{name}: max |hip - f64| {err:.3g} (e_ref {e_ref:.3g}, allowed {bar:.3g})')
    group = name.split(' ')[-1]
    REPORT['max_err_over_allowed'][group] = max(REPORT['max_err_over_allowed'].get(group, 0.0), err / bar)
    REPORT['elements'] += got.numel()
    assert err <= bar, (name, err, bar)


def _zero_bits(t):
    return torch.equal(t.contiguous().view(torch.int32), torch.zeros(t.shape, dtype=torch.int32, device=t.device))


def one_body_library():
    """A skeleton of one body with one three-dof joint on it: three clips of 2, 3 and 7 frames."""
    g = R._gen(7)
    nfs, fps = [2, 3, 7], [30, 60, 30]
    parts = {k: [] for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs')}
    for nf in nfs:
        parts['gts'].append(torch.randn(nf, 1, 3, generator=g, dtype=torch.float64))
        parts['grs'].append(R._pattern('generic', nf, False, g).view(nf, 1, 4))
        parts['lrs'].append(R._pattern('generic', nf, False, g).view(nf, 1, 4))
        for k, w in (('grvs', 3), ('gravs', 3), ('dvs', 3)):
            parts[k].append(torch.randn(nf, w, generator=g, dtype=torch.float64))
    clips = {k: torch.cat(v).float() for k, v in parts.items()}
    nf_t = torch.tensor(nfs)
    clips.update(num_frames=nf_t.to(torch.int32), length_starts=(torch.cumsum(nf_t, 0) - nf_t).to(torch.int32),
                 dt=torch.tensor([1.0 / f for f in fps], dtype=torch.float64).float(),
                 lengths=torch.tensor([1.0 / f * (nf - 1) for nf, f in zip(nfs, fps)], dtype=torch.float64).float(),
                 dof_body_ids=[0], dof_offsets=[0, 3], key_body_ids=[])
    return clips


# ---- 1. the recorded cases ---------------------------------------------------------------------------------------------------------
def test_sync_and_reset_on_the_recorded_cases(be, G):
    for i, (name, c) in enumerate(G['cases'].items()):
        clips, n = RV.sub_library(G['clips'], c['m']), c['n']
        k = E.Case(_dev(clips), n, DEV, interleaved=i % 2 == 0)
        k.set(c['motion_ids'], c['progress'])
        k.sync(be, c['motion_dt'])
        torch.cuda.synchronize()
        assert k.sentinels_ok(), name
        assert k.reset.tolist() == c['reset'] and k.terminate.tolist() == c['terminate'], name
        s64 = RV.sync(clips, I64(c['motion_ids']), I64(c['progress']), c['motion_dt'], torch.float64)
        for g, (key, cols) in RV.GROUPS.items():
            _within(f'{name} {g}', (k.root if key == 'root' else k.dof_pos)[:, cols], s64[key][:, cols], c['e_ref'][g])
        assert _zero_bits(k.root[:, 7:]) and _zero_bits(k.dof_vel) and _zero_bits(k.body['body_vel']) and _zero_bits(k.body['body_ang_vel'])
        before = k.snapshot()
        k.advance(be)
        torch.cuda.synchronize()
        after = k.snapshot()
        assert all(torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0)) for a, b in zip(before[:-5], after[:-5])), (name, 'RESET wrote state')
        assert k.motion_ids.tolist() == c['motion_ids_after'] and k.progress.tolist() == c['progress_after'], name
        assert not bool(k.reset.any()) and not bool(k.terminate.any()) and k.ids_out.tolist() == [e if c['reset'][e] else -1 for e in range(n)]
        assert k.sentinels_ok(), name
        REPORT['cases'] += 1


# ---- 2. shapes where it can go wrong: bitwise the sampler entry ------------------------------------------------------------------
@pytest.mark.parametrize('interleaved', (True, False))
@pytest.mark.parametrize('B', (1, 17))
@pytest.mark.parametrize('n', (1, 63, 64, 65, 70))
def test_sync_is_bitwise_motion_state(be, G, n, B, interleaved):
    # synthetic clips only: their frames are 0.02 .. 0.04 rad apart, far from slerp's 0.001 midpoint threshold, so the f32 and the
    # f64 statement take the same branch for every body (the shipped clip's bodies are in the recorded cases, with their e_ref)
    clips = RV.sub_library(G['clips'], 2) if B == 17 else one_body_library()
    dc = _dev(clips)
    M = clips['lengths'].numel()
    g = R._gen(100 * n + B)
    ids = torch.arange(n) % M
    mdt = 1.0 / 60.0
    progress = (torch.rand(n, generator=g) * 1.5 * clips['lengths'][ids] / mdt).long()
    k = E.Case(dc, n, DEV, interleaved=interleaved, actors=3)
    k.set(ids, progress)
    k.sync(be, mdt)
    torch.cuda.synchronize()
    assert k.sentinels_ok()
    t = (progress * mdt).to(DEV)
    ids32 = ids.to(torch.int32).to(DEV)
    rp, rq, dp, rv, rw, dv, kp = be.motion_state(dict(dc, key_body_ids=list(range(B))), ids32, t)
    rp0, rq0, dp0 = be.motion_state(dict(dc, key_body_ids=[]), ids32, t)[:3]                 # n_key 0
    assert torch.equal(k.root[:, 0:3], rp) and torch.equal(k.root[:, 3:7], rq) and torch.equal(k.dof_pos, dp) and torch.equal(k.body['body_pos'], kp)
    assert torch.equal(rp0, rp) and torch.equal(rq0, rq) and torch.equal(dp0, dp)
    assert _zero_bits(k.root[:, 7:]) and _zero_bits(k.dof_vel) and _zero_bits(k.body['body_vel']) and _zero_bits(k.body['body_ang_vel'])
    assert torch.equal(k.body['body_pos'][:, 0], k.root[:, 0:3]) and torch.equal(k.body['body_rot'][:, 0], k.root[:, 3:7])
    s32, s64 = (RV.sync(clips, ids, progress, mdt, dt) for dt in (torch.float32, torch.float64))
    assert k.reset.cpu().tolist() == s32['reset'].tolist() and not bool(k.terminate.any())
    e_ref = float((s32['body_rot'].double() - s64['body_rot']).abs().max())
    assert e_ref <= 1e-4, 'the f32 statement itself is beyond the cap of the generator'
    _within(f'n{n} B{B} body_rot', k.body['body_rot'], s64['body_rot'], e_ref)
    # without the optional outputs the same root and dofs
    k2 = E.Case(dc, n, DEV, interleaved=interleaved, bodies=False)
    k2.set(ids, progress)
    k2.sync(be, mdt)
    torch.cuda.synchronize()
    assert k2.sentinels_ok() and torch.equal(k2.root, k.root) and torch.equal(k2.dof_pos, k.dof_pos) and _zero_bits(k2.dof_vel)
    REPORT['cases'] += 1


# ---- 3. planted rows ---------------------------------------------------------------------------------------------------------------
def test_reset_word_at_the_planted_ties(be, G):
    clips = dict(RV.sub_library(G['clips'], 2))
    mdt = 2 * (1.0 / 60.0)
    t = I64([1, 1]) * mdt
    for length, want in ((t.clone(), [0, 0]), (torch.nextafter(t, torch.zeros(2)), [1, 1]), (torch.nextafter(t, torch.ones(2)), [0, 0])):
        clips['lengths'] = length
        k = E.Case(_dev(clips), 2, DEV)
        k.set([0, 1], [1, 1])
        k.sync(be, mdt)
        torch.cuda.synchronize()
        assert k.reset.tolist() == want and k.terminate.tolist() == [0, 0] and k.sentinels_ok()


def test_rows_outside_the_library_and_id_lists(be, G):
    clips = _dev(RV.sub_library(G['clips'], 2))
    n = 70
    ids = [e % 2 for e in range(n)]
    bad = {2: 2, 4: -1, 64: 5, 69: 1 << 30}
    for e, v in bad.items():
        ids[e] = v
    flags = [int(e % 3 != 1) for e in range(n)]
    k = E.Case(clips, n, DEV)
    k.set(ids, list(range(n)), reset=flags)
    k.sync(be, 1.0 / 60.0)
    torch.cuda.synchronize()
    good = [e for e in range(n) if e not in bad]
    assert k.sentinels_ok(rows=good)
    assert [int(k.reset[e]) for e in bad] == [flags[e] for e in bad] and [int(k.terminate[e]) for e in bad] == [7] * 4
    # due mode: a row that is not due, or whose id is outside the library, is untouched bit for bit
    k.set(ids, list(range(n)), reset=flags)
    k.advance(be)
    torch.cuda.synchronize()
    due = [bool(flags[e]) and e not in bad for e in range(n)]
    assert k.ids_out.tolist() == [e if due[e] else -1 for e in range(n)]
    assert k.motion_ids.tolist() == [(ids[e] + n) % 2 if due[e] else ids[e] for e in range(n)]
    assert k.progress.tolist() == [0 if due[e] else e for e in range(n)]
    assert k.reset.tolist() == [0 if due[e] else flags[e] for e in range(n)] and k.terminate.tolist() == [0 if due[e] else 7 for e in range(n)]
    # an id list with -1 rows and ids outside the buffers
    k.set([0] * n, list(range(n)), reset=5, terminate=6)
    k.ids_out.fill_(E.ISENT)
    lst = [3, -1, 0, n, 68, -5, 64, (1 << 31) - 1]
    k.advance(be, env_ids=torch.tensor(lst, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    hit = {3, 0, 68, 64}
    assert k.motion_ids.tolist() == [0] * n                                    # (0 + 70) mod 2
    assert k.progress.tolist() == [0 if e in hit else e for e in range(n)]
    assert k.reset.tolist() == [0 if e in hit else 5 for e in range(n)] and k.terminate.tolist() == [0 if e in hit else 6 for e in range(n)]
    assert k.ids_out.tolist() == [E.ISENT] * n and k.sentinels_ok(rows=good)
    k2 = E.Case(_dev(RV.sub_library(G['clips'], 5)), 3, DEV)
    k2.set([0, 1, 2], [4, 5, 6], reset=[1, 0, 1])
    k2.advance(be, export=False)
    torch.cuda.synchronize()
    assert k2.motion_ids.tolist() == [3, 1, 0] and k2.progress.tolist() == [0, 5, 0] and k2.ids_out.tolist() == [E.ISENT] * 3


def test_operator_equals_the_backend_method(be, G):
    clips = _dev(RV.sub_library(G['clips'], 5))
    n = 65
    ids, progress = torch.arange(n) % 5, torch.arange(n) % 9
    a, b = E.Case(clips, n, DEV), E.Case(clips, n, DEV)
    for k in (a, b):
        k.set(ids, progress)
    a.sync(be, 1.0 / 30.0)
    tail = (clips['gts'], clips['grs'], clips['lrs'], clips['lengths'], clips['num_frames'], clips['dt'], clips['length_starts'],
            clips['dof_body_ids'], clips['dof_offsets'])
    torch.ops.ase_hip.motion_sync('sync', b.motion_ids, b.progress, b.reset, b.terminate, 1.0 / 30.0, b.root, b.dof_pos, b.dof_vel,
                                  b.body['body_pos'], b.body['body_rot'], b.body['body_vel'], b.body['body_ang_vel'], None, None, *tail)
    a.advance(be)
    torch.ops.ase_hip.motion_sync('reset', b.motion_ids, b.progress, b.reset, b.terminate, 0.0, None, None, None, None, None, None, None,
                                  None, b.ids_out, *tail)
    torch.cuda.synchronize()
    assert bool(a.ids_out.ge(0).any()) and a.sentinels_ok() and b.sentinels_ok()
    for x, y in zip(a.snapshot(), b.snapshot()):
        assert torch.equal(x.nan_to_num(nan=7.0), y.nan_to_num(nan=7.0))
    with pytest.raises(RuntimeError):
        torch.ops.ase_hip.motion_sync('play', b.motion_ids, b.progress, b.reset, b.terminate, 0.0, None, None, None, None, None, None, None,
                                      None, None, *tail)
    with pytest.raises(AssertionError):
        be.motion_sync(clips, a.motion_ids.cpu(), a.progress, a.reset, a.terminate, L.MOTION_RESET)


# ---- 4. the environment, end to end ------------------------------------------------------------------------------------------------
def _same(x, y):
    return torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0)) if x.dtype.is_floating_point else torch.equal(x, y)


def test_env_is_consistent_end_to_end(be, G):
    """8 environments, 2 clips, a dozen steps across a clip end: the AMP frame stored at step k + 1 is bitwise build_amp_obs of
    motion_state at step k's (ids, t) with the velocities zeroed; fused is bitwise fused=False."""
    clips = RV.sub_library(G['clips'], 2)
    runs = [E.run_env(E.make_env(be, DEV, clips, 8, fused), 12, device=DEV) for fused in (True, False)]
    for k, (a, b) in enumerate(zip(*runs)):
        for key in a:
            assert _same(a[key], b[key]), f'step {k}: {key} differs between the fused and the unfused step'
    recs = runs[0]
    assert sum(int(r['dones'].sum()) for r in recs) >= 8 and not any(bool(r['terminate'].any()) for r in recs)
    dc = _dev(clips)
    F = 13 + 6 * 13 + 31 + 3 * len(RV.KEY_BODY_IDS)
    for k in range(len(recs) - 1):
        frame = E.expected_frame(be, dc, recs[k]['sync_ids'], recs[k]['sync_t'], RV.KEY_BODY_IDS, F)
        assert torch.equal(recs[k + 1]['amp_obs'][:, :F], frame), f'the AMP frame of step {k + 1} is not the pose synced at step {k}'
        assert torch.equal(recs[k]['dones'].cpu(), (recs[k]['sync_t'].cpu() > clips['lengths'][recs[k]['sync_ids'].long().cpu()]).long())
    REPORT['cases'] += 1


def test_step_replays_in_a_launch_program(be, G):
    """post_physics_step (env_post_step + the SYNC launch) recorded once and replayed, equal to an eager twin."""
    clips = RV.sub_library(G['clips'], 2)
    a, b = E.make_env(be, DEV, clips, 8, True), E.make_env(be, DEV, clips, 8, True)
    for env in (a, b):
        env.reset()
    prog = be.prog_create()
    be.prog_begin(prog)
    a.post_physics_step()
    be.prog_end(prog)
    torch.cuda.synchronize()
    try:
        assert be.prog_size(prog) >= 2 and not bool(a.progress_buf.any()), 'recording executes nothing'
        for k in range(12):
            be.prog_launch(prog)
            b.post_physics_step()
            a.reset_done()
            b.reset_done()
            torch.cuda.synchronize()
            for x, y in ((a.progress_buf, b.progress_buf), (a.motion_ids, b.motion_ids), (a.physics.root_states, b.physics.root_states),
                         (a.physics.dof_state, b.physics.dof_state), (a.physics.rigid_body_state, b.physics.rigid_body_state),
                         (a.amp.amp_obs_buf, b.amp.amp_obs_buf), (a.obs_buf, b.obs_buf), (a.reset_ids, b.reset_ids)):
                assert _same(x, y), k
        assert int(a.progress_buf.max()) < 12                     # some rows went past their clip and were reset
    finally:
        be.prog_destroy(prog)
