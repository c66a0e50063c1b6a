"""The demo fetch on the MI355X: ``ase_hip_amp_demo_fetch`` through ``HipBackend``, ``AmpObsDemoSource.fetch_into``,
``torch.ops.ase_hip.amp_demo_fetch``, a launch program, ``ReplayBuffer.store_with`` and ``AMPAgent`` with ``device_demo_fetch``.
Every comparison is bitwise: the observations against the existing two-launch chain (``build_amp_obs_demo``: ``ase_hip_motion_state``
+ ``ase_hip_build_amp_obs``, pinned to f64 references by tests/test_gpu_amp_obs.py) on the same clips and times, the exported draws
against the numpy statement of the draw table (tests/ref_amp_demo.py).  Outputs live in longer NaN- / sentinel-filled allocations
whose guard words are checked after every launch, so rows and columns outside the destination are part of every comparison."""
import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd.learning.replay_buffer import ReplayBuffer
from ase_amd.motion_lib import AmpObsDemoSource, DeviceMotionLib
from tests import ref_amp_demo as RD
from tests import ref_amp_obs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -77
FLAGS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(DEV)


@pytest.fixture(scope='module', autouse=True)
def _report():
    before = dict(R.COUNTS)
    yield
    print('\namp_demo_fetch: comparisons', {k: R.COUNTS[k] - before[k] for k in before}, '(every one asserted bitwise equal)')


def _lib(be, clips=None, weights=None, seed=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return DeviceMotionLib.from_arrays(R.motion_library() if clips is None else clips, be, DEV, weights=weights, generator=gen)


def _source(be, ml, S=RD.STEPS, flags=(True, True), seed=RD.SEED):
    return AmpObsDemoSource(ml, be, num_amp_obs_steps=S, dt=RD.DT, local_root_obs=flags[0], root_height_obs=flags[1], seed=seed)


def _iwindow(n):
    """int32 [n] inside a sentinel-filled allocation -> (view, whole)."""
    whole = torch.full((n + 2 * R.GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return whole[R.GUARD:R.GUARD + n], whole


def _iguards(whole, n, what):
    g = torch.cat([whole[:R.GUARD], whole[R.GUARD + n:]]).cpu()
    R.COUNTS['sentinels'] += g.numel()
    assert bool((g == SENTINEL).all()), f'{what}: a guard word was written'


def _chain(be, src, ids, t0):
    """The existing chain on (ids, t0) -> [n, S F] (a copy).  More than 32 key bodies: ``ase_hip_motion_state`` takes at most 32,
    so the key bodies go through it in two halves - a key body's position does not depend on the others."""
    ml, S = src._motion_lib, src._num_amp_obs_steps
    n, keys = ids.shape[0], ml.clips['key_body_ids']
    if len(keys) <= 32:
        return src.build_amp_obs_demo(ids.long(), t0).reshape(n, -1).clone()
    idx = ids.long().view(-1, 1).expand(n, S).reshape(-1).to(torch.int32)
    times = (t0.unsqueeze(-1) + (-src.dt * torch.arange(0, S, device=DEV))).reshape(-1)        # as build_amp_obs_demo
    half = len(keys) // 2
    parts = [be.motion_state(dict(ml.clips, key_body_ids=k), idx, times) for k in (keys[:half], keys[half:])]
    root_pos, root_rot, dof_pos, root_vel, root_ang_vel, dof_vel, _ = parts[0]
    key_pos = torch.cat([parts[0][6], parts[1][6]], dim=1).contiguous()
    frames = torch.zeros(n * S, 1, src._num_amp_obs_per_step, device=DEV)
    be.build_amp_obs(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_pos, ml.clips['dof_offsets'],
                     src._local_root_obs, src._root_height_obs, frames, shift=False)
    return frames.view(n, -1).clone()


def _fetch_plain(src, n, what, **kw):
    """fetch_into a plain [n, S F] window -> the rows, guards checked."""
    out, whole = R.window((n, src.get_num_amp_obs()), DEV)
    src.fetch_into(out, n, 0, n, **kw)
    torch.cuda.synchronize()
    R.guards_intact(whole, out.numel(), what)
    return out


def _seeded_draws(ml, src, n):
    """ids / t0 as fetch_amp_obs_demo draws them, then the planted times: exactly truncate_time, exactly the clip's length, and
    a clip shorter than truncate_time (its slots reach negative times)."""
    S = src._num_amp_obs_steps
    tr = src.dt * (S - 1)
    ids = ml.sample_motions(n)
    t0 = ml.sample_time(ids, truncate_time=tr) + tr
    if n >= 3:
        lengths = ml.clips['lengths']
        ids[0], t0[0] = 3, tr                                  # (float32(tr): what the sum above gives for phase 0)
        ids[1], t0[1] = 2, lengths[2]
        ids[2] = 0                                             # what the draw table gives this clip at u = 0.5, in f32
        t0[2] = (lengths[0] - tr) * 0.5 + tr
    return ids.to(torch.int32).contiguous(), t0.contiguous()


# ---- 1. passed-in draws = the existing chain --------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('S', [1, 2, 10])
def test_passed_in_draws_equal_the_chain(be, S, flags):
    ml = _lib(be)
    src = _source(be, ml, S, flags)
    for n in R.MOTION_N:                                       # 1 / 63 / 64 / 65 / 130
        ids, t0 = _seeded_draws(ml, src, n)
        if n >= 3 and S == 10:
            times = RD.slot_times(t0.cpu().numpy(), RD.DT, S)
            assert (times[2] < 0).any() and float(t0[2]) > float(ml.clips['lengths'][0])
            assert t0[0].item() == RD.truncate_time(RD.DT, S) and t0[1].item() == ml.clips['lengths'][2].item()
        want = _chain(be, src, ids, t0)
        got = _fetch_plain(src, n, f'n{n} S{S} {flags}', motion_ids=ids, motion_times0=t0)
        R.bitwise(got, want, f'passed-in draws n{n} S{S} {flags}')
        R.COUNTS['cases'] += 1
    assert src.rng_state.tolist() == [RD.SEED, 0]              # passed-in draws leave the stream alone


# ---- 2. layouts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout,S,n', [('humanoid', 10, 65), ('hinge1', 10, 65), ('f255', 10, 65), ('k0', 10, 65), ('f255', 32, 3),
                                        ('hinge1', 40, 3)])
def test_layouts(be, layout, S, n):
    """The humanoid table, one hinge + one key, F = 255 with 34 key bodies (the largest tile: 32 slots of it are the most that
    fit), no key bodies; more than 32 slots: a sample per block."""
    clips = RD.layout_library(layout)
    ml = _lib(be, clips)
    src = _source(be, ml, S)
    assert src._num_amp_obs_per_step == R.frame_size(layout)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 3, (n,), generator=g).to(torch.int32).to(DEV)
    t0 = (torch.rand(n, generator=g) * 0.5).to(DEV)            # with up to 39 steps back: interior, before the start, beyond the end
    want = _chain(be, src, ids, t0)
    got = _fetch_plain(src, n, f'{layout} S{S}', motion_ids=ids, motion_times0=t0)
    R.bitwise(got, want, f'layout {layout} S{S}')
    assert bool(torch.isfinite(got).all())
    R.COUNTS['cases'] += 1


# ---- 3. device draws ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', RD.WEIGHTS)
@pytest.mark.parametrize('offset', RD.OFFSETS)
def test_device_draws(be, offset, weights):
    n = 130
    ml = _lib(be, weights=weights)
    src = _source(be, ml)
    src.rng_state[1] = offset
    m, t = RD.ref_draws(RD.SEED, offset, n, ml.clip_cdf.cpu().numpy(), ml.clips['lengths'].cpu().numpy(),
                        RD.truncate_time(RD.DT, RD.STEPS))
    ids, iwhole = _iwindow(n)
    t0, twhole = R.window((n,), DEV)
    got = _fetch_plain(src, n, f'drawn {offset} {weights}', draws_out=(ids, t0), advance=False)
    _iguards(iwhole, n, 'motion_ids_out')
    R.guards_intact(twhole, n, 'motion_times0_out')
    assert torch.equal(ids.cpu(), torch.from_numpy(m)), 'motion_ids_out is not the draw table'
    R.bitwise(t0, torch.from_numpy(t), f'motion_times0_out {offset} {weights}')
    if weights is not None:
        assert set(ids.unique().tolist()) == {1, 3}            # a clip of weight zero is never drawn
    R.bitwise(got, _chain(be, src, ids.clone(), t0.clone()), f'drawn observations {offset} {weights}')
    assert src.rng_state.tolist() == [RD.SEED, offset]         # advance off: the position stays
    again = _fetch_plain(src, n, 'drawn again')                # ... and a second call repeats the first; this one advances
    R.bitwise(again, got, 'the same stream position twice')
    assert src.rng_state.tolist() == [RD.SEED, offset + 1]
    moved = _fetch_plain(src, n, 'drawn at the next position')
    assert not torch.equal(moved, got) and src.rng_state.tolist() == [RD.SEED, offset + 2]
    R.COUNTS['cases'] += 1


# ---- 4. the ring ----------------------------------------------------------------------------------------------------------------
def _ring(ring_rows, ld):
    """A ring inside a NaN-guarded allocation, every element a value of its own."""
    ring, whole = R.window((ring_rows, ld), DEV)
    ring.copy_(torch.arange(ring_rows * ld, dtype=torch.float32, device=DEV).view(ring_rows, ld) * 0.5 - 7.0)
    return ring, whole


@pytest.mark.parametrize('pad', [0, 7])
@pytest.mark.parametrize('head,n', [(0, 30), (90, 30), (99, 30), (0, 100), (90, 100), (99, 100)])
def test_ring_placement(be, head, n, pad):
    ring_rows, S = 100, 2
    ml = _lib(be)
    src = _source(be, ml, S)
    W = src.get_num_amp_obs()
    ids, t0 = _seeded_draws(ml, src, n)
    ids[5], ids[6] = -1, 4                                     # outside the library: the row stays
    rows = _chain(be, src, ids.clamp(0, 3), t0)
    ring, whole = _ring(ring_rows, W + pad)
    want = ring.clone()
    keep = (ids >= 0) & (ids < 4)
    dst = ((head + torch.arange(n, device=DEV)) % ring_rows)
    want[dst[keep], :W] = rows[keep]
    src.fetch_into(ring, ring_rows, head, n, motion_ids=ids, motion_times0=t0)
    torch.cuda.synchronize()
    R.guards_intact(whole, ring.numel(), f'ring head {head} n {n} pad {pad}')
    R.bitwise(ring, want, f'ring head {head} n {n} pad {pad}')
    assert int(keep.sum()) == n - 2
    R.COUNTS['cases'] += 1


# ---- 5. layers ------------------------------------------------------------------------------------------------------------------
def test_torch_op_equals_the_backend_call(be):
    n, ring_rows, head = 30, 40, 25
    ml = _lib(be)
    a, b = _source(be, ml), _source(be, ml)
    W, c = a.get_num_amp_obs(), ml.clips
    ra, wa = _ring(ring_rows, W)
    rb, wb = _ring(ring_rows, W)
    ia, iwa = _iwindow(n)
    ib, iwb = _iwindow(n)
    ta, ttb = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    a.fetch_into(ra, ring_rows, head, n, draws_out=(ia, ta))
    clip = [c[k] for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'num_frames', 'dt', 'length_starts')]
    out = torch.ops.ase_hip.amp_demo_fetch(rb, ring_rows, head, n, RD.STEPS, RD.DT * (RD.STEPS - 1), RD.DT, None, None, b.rng_state,
                                           ml.clip_cdf, ib, ttb, *clip, c['dof_body_ids'], c['dof_offsets'], c['key_body_ids'],
                                           True, True)
    torch.cuda.synchronize()
    assert out is None and a.rng_state.tolist() == b.rng_state.tolist() == [RD.SEED, 1]
    for w_, k in ((wa, 'a'), (wb, 'b')):
        R.guards_intact(w_, ra.numel(), 'torch op ' + k)
    _iguards(iwa, n, 'ids a'); _iguards(iwb, n, 'ids b')
    R.bitwise(rb, ra, 'torch op ring')
    R.bitwise(ttb, ta, 'torch op times')
    assert torch.equal(ia, ib)
    # passed-in draws through the operator
    torch.ops.ase_hip.amp_demo_fetch(rb, ring_rows, 0, n, RD.STEPS, RD.DT * (RD.STEPS - 1), RD.DT, ia.clone(), ta.clone(), None, None,
                                     None, None, *clip, c['dof_body_ids'], c['dof_offsets'], c['key_body_ids'], True, True)
    torch.cuda.synchronize()
    R.bitwise(rb[:n], ra[(head + torch.arange(n, device=DEV)) % ring_rows], 'torch op, passed-in draws')
    with pytest.raises(RuntimeError):                          # half an export
        torch.ops.ase_hip.amp_demo_fetch(rb, ring_rows, head, n, RD.STEPS, 0.3, RD.DT, None, None, b.rng_state, ml.clip_cdf, ib, None,
                                         *clip, c['dof_body_ids'], c['dof_offsets'], c['key_body_ids'], True, True)
    with pytest.raises(RuntimeError):                          # both modes
        torch.ops.ase_hip.amp_demo_fetch(rb, ring_rows, head, n, RD.STEPS, 0.3, RD.DT, ia, ta, b.rng_state, ml.clip_cdf, None, None,
                                         *clip, c['dof_body_ids'], c['dof_offsets'], c['key_body_ids'], True, True)
    R.COUNTS['cases'] += 1


def test_fetch_in_a_launch_program_follows_head_and_offset(be):
    """Recorded once with the ring head in a device word, replayed with the word rewritten: each replay equals an eager call
    with that head at the same stream position.  A head outside the ring writes nothing."""
    n, ring_rows = 30, 100
    ml = _lib(be)
    a, b = _source(be, ml), _source(be, ml)
    W = a.get_num_amp_obs()
    ra, wa = _ring(ring_rows, W)
    rb, wb = _ring(ring_rows, W)
    hd = torch.zeros(1, dtype=torch.int32, device=DEV)
    before = ra.clone()
    prog = be.prog_create()
    be.prog_begin(prog)
    a.fetch_into(ra, ring_rows, 0, n, head_dev=hd)
    be.prog_end(prog)
    torch.cuda.synchronize()
    assert be.prog_size(prog) == 2                             # the fetch and the stream position
    R.bitwise(ra, before, 'recorded, not executed')
    assert a.rng_state.tolist() == [RD.SEED, 0]
    for i, head in enumerate((0, 95, 40, 99)):
        hd.fill_(head)
        be.prog_launch(prog)
        b.fetch_into(rb, ring_rows, head, n)
        torch.cuda.synchronize()
        assert a.rng_state.tolist() == b.rng_state.tolist() == [RD.SEED, i + 1]
        R.guards_intact(wa, ra.numel(), f'replay {i}')
        R.bitwise(ra, rb, f'replay {i}, head {head}')
    kept = ra.clone()
    for bad in (-1, ring_rows):
        hd.fill_(bad)
        be.prog_launch(prog)
        torch.cuda.synchronize()
        R.guards_intact(wa, ra.numel(), f'head word {bad}')
        R.bitwise(ra, kept, f'head word {bad}: nothing written')
    assert a.rng_state.tolist() == [RD.SEED, 6]                # a call is one stream position, whatever it wrote
    be.prog_destroy(prog)
    R.COUNTS['cases'] += 1


def test_store_with_equals_store_of_the_same_draws(be):
    ml = _lib(be)
    src = _source(be, ml, S=2)
    W = src.get_num_amp_obs()
    a, b = ReplayBuffer(100, DEV, be), ReplayBuffer(100, DEV, be)
    for n in (30, 30, 30, 30, 100):                            # the fourth store wraps
        ids, t0 = _seeded_draws(ml, src, n)
        a.store_with(lambda data, rr, h, k: src.fetch_into(data, rr, h, k, motion_ids=ids, motion_times0=t0), n, W)
        b.store(_chain(be, src, ids, t0))
        torch.cuda.synchronize()
        assert (a._head, a._total_count) == (b._head, b._total_count)
        R.bitwise(a.data, b.data, f'store_with after {a._total_count} rows')
    assert a._head == 20 and a._total_count == 220
    R.COUNTS['cases'] += 1


@pytest.fixture
def boundary(monkeypatch):
    import tests.test_boundary_emu as T
    from ase_amd.backend import HipBackend
    monkeypatch.setattr(T, '_DEV', DEV)
    monkeypatch.setattr(T, '_BE', lambda: HipBackend(DEV))
    return T


def test_agent_with_device_demo_fetch(boundary, golden_dir, monkeypatch):
    from ase_amd.synthetic import EnvSpec, SyntheticVecEnv
    T = boundary
    G = T._load(golden_dir, 'amp')
    hb = T._BE()
    s = G['spec']
    spec = EnvSpec(num_envs=s['num_envs'], horizon=G['cfg']['horizon_length'], obs_size=s['obs_size'], act_size=s['act_size'],
                   amp_obs_size=s['amp_obs_size'], episode_length=5)
    ml = DeviceMotionLib.from_arrays(RD.tiny_library(), hb, DEV)
    src = AmpObsDemoSource(ml, hb, num_amp_obs_steps=RD.TINY_STEPS, dt=RD.DT, seed=RD.SEED)
    env = SyntheticVecEnv(spec, seed=3, device=DEV, demo_source=src)
    ag, _ = T._agent(G, env, be=hb, device_demo_fetch=True)
    ring = ag._amp_obs_demo_buffer
    size, batch, W = ring.get_buffer_size(), ag._amp_batch_size, src.get_num_amp_obs()
    ag._init_amp_demo_buf()
    torch.cuda.synchronize()
    assert ring.get_total_count() == size and src.rng_state.tolist() == [RD.SEED, size // batch]
    # every refill is the chain on the draw table of its stream position
    for i in range(size // batch):
        m, t = RD.ref_draws(RD.SEED, i, batch, ml.clip_cdf.cpu().numpy(), ml.clips['lengths'].cpu().numpy(),
                            RD.truncate_time(RD.DT, RD.TINY_STEPS))
        want = _chain(hb, src, torch.from_numpy(m).to(DEV), torch.from_numpy(t).to(DEV))
        R.bitwise(ring.data[i * batch:(i + 1) * batch], want, f'agent ring, refill {i}')
    update = ag._update_amp_demos

    def guarded_update():
        def no(*a, **k):
            raise AssertionError('torch.multinomial called on the device demo path')
        with monkeypatch.context() as mp:
            mp.setattr(torch, 'multinomial', no)
            update()
    ag._update_amp_demos = guarded_update
    ag.obs = ag.env_reset()
    info = ag.train_epoch()
    torch.cuda.synchronize()
    assert ring.get_total_count() == size + batch and ring._head == batch and src.rng_state.tolist() == [RD.SEED, size // batch + 1]
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in info['disc_loss'])
    R.COUNTS['cases'] += 1
