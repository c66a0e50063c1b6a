"""The demo fetch without a GPU: the host-side operand checks of ``ase_hip_amp_demo_fetch``, the numpy draw table
(tests/ref_amp_demo.py) against its definition, the conditions the GPU file's fixtures promise, the ring placement of the CPU
stand-in (tests/emu_amp_demo.py), ``ReplayBuffer.store_with`` and the agents' ``device_demo_fetch`` on the stand-in."""
import ctypes

import numpy as np
import pytest
import torch

from ase_amd import lib as L
from ase_amd.learning.replay_buffer import ReplayBuffer
from ase_amd.motion_lib import AmpObsDemoSource, DeviceMotionLib, clip_cdf
from ase_amd.synthetic import EnvSpec, SyntheticVecEnv
from tests import ref_amp_demo as RD
from tests import ref_amp_obs as R
from tests import ref_rollout as RR
from tests import test_boundary_emu as T
from tests.emu_amp_demo import EmuAmpDemo


# ---- 1. operand refusals --------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_operands_without_gpu():
    """Every refusal of the C entry.  Nothing may ever be launched here (the operands are host memory), so the call ALWAYS
    carries a defect the LAST check refuses - 64 slots of a 255-float frame are beyond the 64 KB tile: that message proves that
    every earlier check let the operands pass, and an earlier defect is named by its own message."""
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ase_hip_last_error()
    ia = lambda *xs: (ctypes.c_int32 * len(xs))(*xs)
    J, K = 20, 34                                              # 13 + 120 + 20 + 102 = 255 floats

    def fetch(**kw):
        a = dict(gts=p, grs=p, lrs=p, grvs=p, gravs=p, dvs=p, n_bodies=40, lengths=p, num_frames=p, dt=p, length_starts=p, n_clips=4,
                 dof_body_ids=ia(*range(1, J + 1)), offs=ia(*range(J + 1)), n_joints=J, key_ids=ia(*range(K)), n_key=K,
                 motion_ids=p, times0=p, rng=None, cdf=None, advance=1, ids_out=None, times_out=None, n=30, n_steps=64, trunc=0.3,
                 step_dt=1.0 / 30.0, local=1, height=1, out=p, ld_out=64 * 255, ring_rows=100, head=0, head_dev=None)
        a.update(kw)
        return lib.ase_hip_amp_demo_fetch(a['gts'], a['grs'], a['lrs'], a['grvs'], a['gravs'], a['dvs'], a['n_bodies'], a['lengths'],
                                          a['num_frames'], a['dt'], a['length_starts'], a['n_clips'], a['dof_body_ids'], a['offs'],
                                          a['n_joints'], a['key_ids'], a['n_key'], a['motion_ids'], a['times0'], a['rng'], a['cdf'],
                                          a['advance'], a['ids_out'], a['times_out'], a['n'], a['n_steps'], a['trunc'], a['step_dt'],
                                          a['local'], a['height'], a['out'], a['ld_out'], a['ring_rows'], a['head'], a['head_dev'], None)

    last = b'do not fit the staging tile'
    passes = lambda **kw: fetch(**kw) == -1 and last in err()
    assert passes()                                                                    # the defaults reach the last check
    dev = dict(motion_ids=None, times0=None, rng=p, cdf=p)                              # the other mode
    assert passes(**dev)
    # null operands, per mode
    for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'num_frames', 'dt', 'length_starts', 'dof_body_ids', 'offs',
              'key_ids', 'out'):
        assert fetch(**{k: None}) == -1 and b'amp_demo_fetch: null operand' in err(), k
        assert fetch(**dict(dev, **{k: None})) == -1 and b'amp_demo_fetch: null operand' in err(), k
    # without key bodies a NULL key_body_ids passes: 13 + 6 * 32 + 32 = 237 floats, 64 slots of them are still too many
    assert passes(key_ids=None, n_key=0, n_joints=32, offs=ia(*range(33)), dof_body_ids=ia(*([1] * 32)), ld_out=64 * 237)
    assert fetch(times0=None) == -1 and b'need motion_ids and motion_times0' in err()
    assert fetch(motion_ids=None) == -1 and b'need motion_ids and motion_times0' in err()
    assert fetch(**dict(dev, cdf=None)) == -1 and b'need rng_state and cdf' in err()
    assert fetch(**dict(dev, rng=None)) == -1 and b'need rng_state and cdf' in err()
    # both modes at once, or neither
    assert fetch(rng=p, cdf=p) == -1 and b'at once' in err()
    assert fetch(rng=p) == -1 and b'at once' in err()
    assert fetch(motion_ids=None, times0=None) == -1 and b'neither' in err()
    # the export comes both or none, in either mode
    assert fetch(ids_out=p) == -1 and b'both or none' in err()
    assert fetch(times_out=p) == -1 and b'both or none' in err()
    assert fetch(**dict(dev, ids_out=p)) == -1 and b'both or none' in err()
    assert passes(ids_out=p, times_out=p) and passes(**dict(dev, ids_out=p, times_out=p))
    # sizes
    for n in (0, -1):
        assert fetch(n=n) == -1 and b'bad sizes (n %d' % n in err()
    assert passes(n=1)
    assert fetch(n_clips=0) == -1 and b'clips 0' in err()
    assert passes(n_clips=1)
    assert fetch(n_bodies=0) == -1 and b'bad sizes' in err()
    for s in (0, -1, 65):
        assert fetch(n_steps=s) == -1 and b'n_steps %d (1-64' % s in err()
    assert fetch(n=101) == -1 and b'n 101 does not fit a ring of 100 rows' in err()
    assert passes(n=100) and passes(n=100, head=99)
    assert fetch(ring_rows=0, n=1) == -1 and b'does not fit' in err()
    for h in (-1, 100):
        assert fetch(head=h) == -1 and b'head %d outside [0, 100)' % h in err()
    assert passes(head=99)
    assert fetch(ld_out=64 * 255 - 1) == -1 and b'ld_out 16319 below' in err()
    assert passes(ld_out=64 * 255 + 7)
    # the character
    assert fetch(n_joints=0) == -1 and b'0 joints' in err()
    assert fetch(n_joints=33, offs=ia(*range(34)), dof_body_ids=ia(*([1] * 33))) == -1 and b'33 joints' in err()
    assert fetch(n_key=-1) == -1 and fetch(n_key=79, key_ids=ia(*([0] * 79))) == -1 and b'79 key bodies' in err()
    assert fetch(offs=ia(0, 2, *range(3, J + 2))) == -1 and b'joint 0 has 2 dofs' in err()
    assert fetch(offs=ia(*range(J), J + 3)) == -1 and b'joint 19 has 4 dofs' in err()
    assert fetch(offs=ia(1, *range(1, J + 1))) == -1 and b'do not cover' in err()                       # dof_offsets[0] != 0
    assert fetch(dof_body_ids=ia(40, *range(2, J + 1))) == -1 and b'joint 0 on body 40 of 40' in err()
    assert fetch(dof_body_ids=ia(*range(1, J), -1)) == -1 and b'joint 19 on body -1' in err()
    assert passes(dof_body_ids=ia(39, *range(2, J + 1)))
    assert fetch(key_ids=ia(*range(K - 1), 40)) == -1 and b'key body 40 out of range' in err()
    assert fetch(key_ids=ia(-1, *range(1, K))) == -1 and b'key body -1 out of range' in err()
    # F = 13 + 6 J + D + 3 K: 255 floats pass, 256 are refused (one 3-dof joint more than hinges: D = 22, one key body fewer)
    wide = ia(0, 3, *range(4, J + 3))
    assert fetch(offs=wide, n_key=K - 1) == -1 and b'frame of 254 floats' not in err() and last in err()
    assert fetch(offs=ia(*range(J + 1)), n_key=K + 1, key_ids=ia(*range(K + 1))) == -1 and b'frame of 258 floats' in err()
    assert fetch(offs=wide, n_key=K) == -1 and b'frame of 257 floats' in err() and b'at most 255' in err()
    # the tile check is the last one: 64 slots of 255 floats are refused (the defaults).  That 32 slots of them fit cannot be
    # shown without a launch; tests/test_gpu_amp_demo.py runs that shape.


def test_torch_op_is_registered():
    import ase_amd.ops  # noqa: F401
    schema = str(torch.ops.ase_hip.amp_demo_fetch.default._schema)
    assert schema.startswith('ase_hip::amp_demo_fetch(Tensor(a0!) out, ') and schema.endswith('-> ()')
    for name in ('rng_state', 'motion_ids_out', 'motion_times0_out'):          # written in place, each optional
        assert f'!)? {name}' in schema, (name, schema)
    assert 'Tensor? motion_ids, Tensor? motion_times0' in schema and 'Tensor? head_dev=None' in schema
    with pytest.raises(NotImplementedError):                                   # no CPU kernel: the product has no fallback
        torch.ops.ase_hip.amp_demo_fetch(torch.zeros(4, 44), 4, 0, 4, 2, 0.1, 0.1, None, None, None, None, None, None,
                                         *[torch.zeros(1)] * 10, [1], [0, 3], [], True, True)


# ---- 2. the draw table ----------------------------------------------------------------------------------------------------------
def _lengths():
    return R.motion_library()['lengths'].numpy()


def test_draw_table_against_its_definition():
    """Element 2 i of the stream gives the clip through cdf, element 2 i + 1 the time, in f32 operation by operation."""
    n, lengths = 4096, _lengths()
    tr = RD.truncate_time(RD.DT, RD.STEPS)
    assert tr == np.float32(0.3) and lengths[0] < tr and lengths[1] < tr and lengths[2] > tr and lengths[3] > tr
    for w in RD.WEIGHTS:
        wt = torch.ones(4) if w is None else torch.tensor(w)
        cdf = clip_cdf(wt / wt.sum()).numpy()
        for off in RD.OFFSETS:
            m, t0 = RD.ref_draws(RD.SEED, off, n, cdf, lengths, tr)
            assert m.dtype == np.int32 and t0.dtype == np.float32
            for i in (0, 1, 77, n - 1):                        # the table, element by element
                w0 = RR.philox4x32_10(2 * i, off, RD.SEED)
                w1 = RR.philox4x32_10(2 * i + 1, off, RD.SEED)
                v = int(w0[2][0]) >> 8
                mi = next(k for k in range(4) if v < int(cdf[k]))
                u = np.float32(int(w1[2][0]) >> 8) * np.float32(2.0 ** -24)
                want = np.float32(np.float32(u * np.float32(lengths[mi] - tr)) + tr)
                assert int(m[i]) == mi and t0[i].tobytes() == want.tobytes()
            if w is not None:                                  # a clip of weight zero is never drawn
                assert set(np.unique(m).tolist()) == {1, 3}
                assert abs(float((m == 3).mean()) - 2.0 / 3.0) < 0.03
            else:
                assert set(np.unique(m).tolist()) == {0, 1, 2, 3}
            long_ = lengths[m] >= tr
            assert long_.any() and (t0[long_] >= tr).all() and (t0[long_] <= lengths[m][long_]).all()
            short = ~long_                                     # u * (negative span) + trunc: between the length and trunc
            assert short.any() and (t0[short] <= tr).all() and (t0[short] > lengths[m][short]).all()
    # another stream position, other draws; seed and offset above 2^32 both reach the counter
    a = RD.ref_draws(RD.SEED, RD.OFFSETS[0], 64, cdf, lengths, tr)
    b = RD.ref_draws(RD.SEED, RD.OFFSETS[1], 64, cdf, lengths, tr)
    c = RD.ref_draws(RD.SEED & 0xFFFFFFFF, RD.OFFSETS[0], 64, cdf, lengths, tr)
    d = RD.ref_draws(RD.SEED, RD.OFFSETS[1] & 0xFFFFFFFF, 64, cdf, lengths, tr)
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(a[1], c[1]) and not np.array_equal(b[1], d[1])
    assert RD.SEED > 1 << 32 and RD.OFFSETS[1] > 1 << 32


def test_gpu_fixture_conditions():
    """What tests/test_gpu_amp_demo.py relies on: at n = 130 every clip is drawn at least 8 times and every kind of frame pair
    - interior, the first-frame clamp of a negative time, the last frame paired with itself - is reached by at least 8 items."""
    clips = R.motion_library()
    cdf = clip_cdf(torch.ones(4) / 4).numpy()
    tr = RD.truncate_time(RD.DT, RD.STEPS)
    for off in RD.OFFSETS:
        m, t0 = RD.ref_draws(RD.SEED, off, 130, cdf, clips['lengths'].numpy(), tr)
        assert np.bincount(m, minlength=4).min() >= 8, np.bincount(m, minlength=4)
        times = RD.slot_times(t0, RD.DT, RD.STEPS)
        assert times.shape == (130, RD.STEPS) and np.array_equal(times[:, 0], t0)
        kinds = RD.frame_pair_kinds(clips, m, times)
        counts = np.bincount(kinds.reshape(-1), minlength=3)
        assert counts.min() >= 8, counts
        assert (kinds[m >= 2] == RD.INTERIOR).all()            # the long clips stay inside
        assert (kinds[m < 2, 0] == RD.LAST_FRAME).all() and (kinds[m < 2, -1] == RD.BEFORE_START).all()
    # the weighted library of the GPU file
    cdf = clip_cdf(torch.tensor(RD.WEIGHTS[1]) / 3).numpy()
    m, _ = RD.ref_draws(RD.SEED, 0, 130, cdf, clips['lengths'].numpy(), tr)
    assert set(np.unique(m).tolist()) == {1, 3} and np.bincount(m, minlength=4)[[1, 3]].min() >= 8


# ---- 3. the stand-in: ring placement, store_with, the agents --------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib_source():
    be = EmuAmpDemo()
    ml = DeviceMotionLib.from_arrays(R.motion_library(), be, 'cpu')
    return be, ml, AmpObsDemoSource(ml, be, num_amp_obs_steps=3, dt=RD.DT, seed=RD.SEED)


@pytest.mark.parametrize('ring_rows,head,n,pad', [(20, 0, 7, 0), (20, 15, 7, 0), (20, 19, 20, 0), (7, 0, 7, 5), (20, 18, 7, 5)])
def test_stand_in_places_rows_in_the_ring(lib_source, ring_rows, head, n, pad):
    be, ml, src = lib_source
    W = src.get_num_amp_obs()
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 4, (n,), generator=g).to(torch.int32)
    t0 = torch.rand(n, generator=g) * 0.5
    if n > 2:
        ids[1], ids[2] = -1, 4                                 # outside the library: the row stays
    rows = src.build_amp_obs_demo(ids.clamp(0, 3).long(), t0).view(n, W).clone()
    before = torch.arange((ring_rows + 1) * (W + pad), dtype=torch.float32).view(ring_rows + 1, W + pad)
    ring = before.clone()
    src.fetch_into(ring, ring_rows, head, n, motion_ids=ids, motion_times0=t0)
    want = before.clone()
    for i in range(n):
        if 0 <= int(ids[i]) < 4:
            want[(head + i) % ring_rows, :W] = rows[i]
    assert torch.equal(ring, want) and not torch.equal(ring, before)
    assert src.rng_state.tolist() == [RD.SEED, 0]              # passed-in draws leave the stream alone


def test_stand_in_draws_on_the_stream(lib_source):
    be, ml, src = lib_source
    n, W = 9, src.get_num_amp_obs()
    src.rng_state[1] = 4
    ids, t0 = torch.zeros(n, dtype=torch.int32), torch.zeros(n)
    a = torch.zeros(n, W)
    src.fetch_into(a, n, 0, n, draws_out=(ids, t0), advance=False)
    m, t = RD.ref_draws(RD.SEED, 4, n, ml.clip_cdf.numpy(), ml.clips['lengths'].numpy(), RD.truncate_time(RD.DT, 3))
    assert np.array_equal(ids.numpy(), m) and t0.numpy().tobytes() == t.tobytes() and src.rng_state.tolist() == [RD.SEED, 4]
    assert torch.equal(a, src.build_amp_obs_demo(ids.long(), t0).view(n, W))
    b = src.fetch_amp_obs_demo_device(n)
    assert torch.equal(a, b) and src.rng_state.tolist() == [RD.SEED, 5]
    assert not torch.equal(src.fetch_amp_obs_demo_device(n), b)
    src.rng_state[1] = 0


def test_store_with_moves_head_and_count_as_store(lib_source):
    be, ml, src = lib_source
    W = src.get_num_amp_obs()
    a, b = ReplayBuffer(20, 'cpu', be), ReplayBuffer(20, 'cpu', be)
    g = torch.Generator().manual_seed(6)
    a.store_with(lambda *args: pytest.fail('produce called for no rows'), 0, W)
    assert a.data is None and a._head == 0
    for n in (7, 7, 7, 20, 1):                                # fills, wraps, a whole ring, one row
        ids = torch.randint(0, 4, (n,), generator=g).to(torch.int32)
        t0 = torch.rand(n, generator=g) * 0.5
        seen = []

        def produce(data, ring_rows, head, k):
            seen.append((data is a.data, ring_rows, head, k))
            src.fetch_into(data, ring_rows, head, k, motion_ids=ids, motion_times0=t0)
        head0 = a._head
        a.store_with(produce, n, W)
        b.store(src.build_amp_obs_demo(ids.long(), t0).view(n, W))
        assert seen == [(True, 20, head0, n)]
        assert (a._head, a._total_count) == (b._head, b._total_count) and torch.equal(a.data, b.data)
    assert a._total_count == 42 and a._head == 2
    with pytest.raises(AssertionError):
        a.store_with(lambda *args: None, 21, W)


def _tiny_env(G, be, seed=3):
    """tests/test_boundary_emu._env with demo observations from clips: one slot of the 44-float frame of a one-hinge character
    with eight key bodies (the emulator's sampler indexes with the key-body list, so the list is not empty)."""
    s = G['spec']
    spec = EnvSpec(num_envs=s['num_envs'], horizon=G['cfg']['horizon_length'], obs_size=s['obs_size'], act_size=s['act_size'],
                   amp_obs_size=s['amp_obs_size'], latent_dim=G['cfg'].get('latent_dim', 0),
                   latent_steps_min=G['cfg'].get('latent_steps_min', 1), latent_steps_max=G['cfg'].get('latent_steps_max', 4),
                   episode_length=5)
    ml = DeviceMotionLib.from_arrays(RD.tiny_library(), be, T._DEV)
    src = AmpObsDemoSource(ml, be, num_amp_obs_steps=RD.TINY_STEPS, dt=RD.DT, seed=RD.SEED)
    return SyntheticVecEnv(spec, seed=seed, device=T._DEV, demo_source=src), src


def _forbid(monkeypatch, be):
    def no(name):
        def raiser(*a, **k):
            raise AssertionError(f'{name} called on the device demo path')
        return raiser
    monkeypatch.setattr(torch, 'multinomial', no('torch.multinomial'))
    monkeypatch.setattr(torch, 'rand', no('torch.rand'))
    monkeypatch.setattr(be, 'ring_store', no('ring_store'))


@pytest.mark.parametrize('kind', ['amp', 'ase'])
def test_agent_with_device_demo_fetch(kind, golden_dir, monkeypatch):
    G = T._load(golden_dir, kind)
    be = EmuAmpDemo()
    env, src = _tiny_env(G, be)
    ag, _ = T._agent(G, env, be=be, device_demo_fetch=True)
    ring = ag._amp_obs_demo_buffer
    size, batch, W = ring.get_buffer_size(), ag._amp_batch_size, src.get_num_amp_obs()
    assert ag._device_demo_fetch and size % batch == 0 and size > batch
    calls = []
    fetch = be.amp_demo_fetch

    def counting(*a, **k):
        calls.append((a[2], a[3], a[4]))                       # ring_rows, head, n
        return fetch(*a, **k)
    monkeypatch.setattr(be, 'amp_demo_fetch', counting)
    _forbid(monkeypatch, be)
    ag._init_amp_demo_buf()
    assert calls == [(size, h, batch) for h in range(0, size, batch)]
    assert ring.get_total_count() == size and ring._head == 0 and src.rng_state.tolist() == [RD.SEED, size // batch]
    data = ring.data.clone()
    assert data.shape == (size, W) and bool(torch.isfinite(data).all()) and bool((data != 0).any(dim=1).all())     # every row filled
    # each refill is the device fetch of its stream position
    m, t0 = RD.ref_draws(RD.SEED, 1, batch, src._motion_lib.clip_cdf.numpy(), src._motion_lib.clips['lengths'].numpy(),
                         RD.truncate_time(RD.DT, RD.TINY_STEPS))
    want = src.build_amp_obs_demo(torch.from_numpy(m).long(), torch.from_numpy(t0)).view(batch, W)
    assert torch.equal(data[batch:2 * batch], want)
    ring._head = 2 * batch                                     # (as after two updates)
    ag._update_amp_demos()
    assert calls[-1] == (size, 2 * batch, batch) and ring._head == 3 * batch and ring.get_total_count() == size + batch
    changed = (ring.data != data).any(dim=1)
    assert bool(changed[2 * batch:3 * batch].all()) and int(changed.sum()) == batch
    monkeypatch.undo()
    # an epoch on this path: the update consumes the ring as before
    ag.obs = ag.env_reset()
    info = ag.train_epoch()
    assert ring.get_total_count() == size + 2 * batch and all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in info['disc_loss'])


def test_default_never_touches_the_entry(golden_dir, monkeypatch):
    G = T._load(golden_dir, 'amp')
    be = EmuAmpDemo()
    env, src = _tiny_env(G, be)

    def no(*a, **k):
        raise AssertionError('amp_demo_fetch called without device_demo_fetch')
    monkeypatch.setattr(be, 'amp_demo_fetch', no)
    ag, _ = T._agent(G, env, be=be)
    assert ag._device_demo_fetch is False
    ag._init_amp_demo_buf()
    ag._update_amp_demos()
    ring = ag._amp_obs_demo_buffer
    assert ring.get_total_count() == ring.get_buffer_size() + ag._amp_batch_size and src.rng_state.tolist() == [RD.SEED, 0]


class _WithoutInto:
    """An environment of before: everything of the stand-in but ``fetch_amp_obs_demo_into``."""

    def __init__(self, env):
        self._e = env

    def __getattr__(self, k):
        if k == 'fetch_amp_obs_demo_into':
            raise AttributeError(k)
        v = getattr(self._e, k)
        return self if v is self._e else v


def test_key_without_the_environment_method_is_refused(golden_dir):
    G = T._load(golden_dir, 'amp')
    with pytest.raises(AssertionError, match='fetch_amp_obs_demo_into'):
        T._agent(G, _WithoutInto(T._env(G)), device_demo_fetch=True)
    ag, _ = T._agent(G, _WithoutInto(T._env(G)))                # without the key such an environment still does
    assert ag._device_demo_fetch is False
    plain = T._env(G)                                          # the stand-in without a demo source has the method, and says so
    with pytest.raises(AssertionError, match='demo_source'):
        plain.fetch_amp_obs_demo_into(torch.zeros(4, 44), 4, 0, 4)
