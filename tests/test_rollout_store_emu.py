"""Host side of the one-launch rollout step, without a GPU: the stand-in tests/emu_rollout_store.py on every
case and bound of tests/test_gpu_rollout_store.py against the reference tests/ref_rollout_store.py, every refusal of
``ase_hip_rollout_store`` (no call here launches anything), the fixture conditions of the meter sequences, six wrong
restatements that each miss a bound, and the agents' ``device_rollout`` on the stand-in."""
import ctypes

import pytest
import torch

from ase_amd import lib as L
from ase_amd.learning import agents
from tests import ref_rollout_store as R
from tests import test_boundary_emu as T
from tests.emu_backend import EmuBackend
from tests.emu_rollout_store import EmuRolloutStore

DEV = 'cpu'


@pytest.fixture(scope='module')
def be():
    return EmuRolloutStore()


# ---- the stand-in against the reference: the cases and bounds of the GPU file ------------------------------------------------
def test_widths_pitches_and_paths(be):
    R.check_widths(be, DEV)


@pytest.mark.parametrize('n', R.N_ENVS)
def test_done_patterns_at_every_size(be, n):
    R.check_n_envs(be, DEV, n)


@pytest.mark.parametrize('n_fields', (0, 1, 16))
def test_field_counts(be, n_fields):
    R.check_n_fields(be, DEV, n_fields)


@pytest.mark.parametrize('term_dtype', R.KINDS)
@pytest.mark.parametrize('dones_dtype', R.KINDS)
def test_flag_kinds(be, dones_dtype, term_dtype):
    R.check_kinds(be, DEV, dones_dtype, term_dtype)


def test_non_finite_rewards(be):
    R.check_special(be, DEV)


def test_nullable_groups(be):
    R.check_groups(be, DEV)


def test_device_slot_word(be):
    R.check_slot_word(be, DEV)


@pytest.mark.parametrize('start_size', (0, 60))
@pytest.mark.parametrize('n', (257, 1030))
def test_meter_sequences_and_their_fixture_conditions(be, n, start_size):
    """run_meter_sequence asserts that the six calls contain k == 0, 0 < k < max_size, k >= max_size and a cut `old`."""
    h1 = R.run_meter_sequence(be, DEV, n, start_size)
    h2 = R.run_meter_sequence(be, DEV, n, start_size)
    assert h1 == h2


# ---- wrong restatements -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wrong', R.WRONG)
def test_single_term_wrong_restatements_miss_a_bound(be, wrong):
    """Each of the six, put in the reference's place, is caught by the checks the right one passes on the same calls."""
    def sequence(wrong):
        st = R.Step(DEV, 257, n_slots=2, fields=[(3, 0, False)], seed=71)
        st.start_meter(12.5, 140.25, 60)
        for i, k in enumerate(R.SEQ_DONE_COUNTS):
            st.inputs(R.done_pattern('count', st.n, st.gen, k))
            ref, w0, w = st.run(be, i % 2, -0.5, 0.01, what=f'{wrong} call {i}', wrong=wrong)
            R.check_meter(w0, w, ref, wrong if wrong in ('size_unclipped', 'old_uncut') else None)
    sequence(None)
    with pytest.raises(AssertionError):
        sequence(wrong)


# ---- the C entry's refusals ---------------------------------------------------------------------------------------------------
def test_entry_point_refuses_without_a_launch():
    """Every refusal of ase_hip_rollout_store.  The slot is checked last, so every call here carries slot = -1 beside the defect
    under test: a call whose defect were missed would still be refused for its slot, and nothing is ever launched."""
    lib = L.load()
    assert len(L.SIGNATURES['ase_hip_rollout_store']) == 28
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ase_hip_last_error()

    def call(**kw):
        a = dict(fields=p, n_fields=2, rewards=p, shift=0.0, scale=1.0, rewards_out=p, rewards_ss=16, dones=p, dones_kind=L.KIND_I64,
                 dones_out=p, dones_ss=16, next_values=p, terminate=p, terminate_kind=L.KIND_U8, next_values_out=p,
                 next_values_ss=16, cur_rewards=p, cur_lengths=p, meter=p, max_size=100, workspace=p,
                 workspace_doubles=L.rollout_store_ws(16), done_ids_out=p, n_envs=16, slot=-1, slot_dev=None, n_slots=4, stream=None)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return lib.ase_hip_rollout_store(*a.values())

    def refused(rc, *words):
        return rc == -1 and b'rollout_store' in err() and all(w in err() for w in words)

    none = dict(cur_rewards=None, cur_lengths=None, meter=None, workspace=None)
    # every operand in order but the slot: refused for the slot, so every earlier check let the call pass
    for kw in ({}, dict(n_fields=0, fields=None), dict(n_fields=16), dict(slot_dev=p), dict(rewards_out=None),
               dict(dones_out=None), dict(done_ids_out=None), dict(next_values=None, terminate=None, next_values_out=None),
               none, dict(none, rewards=None, rewards_out=None), dict(dones_kind=L.KIND_F32, terminate_kind=L.KIND_I32)):
        assert refused(call(**kw), b'slot -1'), kw
    assert refused(call(slot=4), b'slot 4') and refused(call(n_slots=0, slot=0), b'slot')
    assert refused(call(dones=None), b'dones')
    assert refused(call(n_envs=0), b'n_envs') and refused(call(n_envs=-2), b'n_envs')
    assert refused(call(n_fields=-1), b'n_fields') and refused(call(n_fields=17), b'n_fields')
    assert refused(call(fields=None), b'without a table')
    assert refused(call(dones_kind=4), b'dones kind') and refused(call(dones_kind=-1), b'dones kind')
    assert refused(call(terminate_kind=7), b'terminate kind')
    for k in ('cur_rewards', 'cur_lengths', 'meter', 'workspace'):
        assert refused(call(**{k: None}), b'partial accumulator group'), k
    for k in ('next_values', 'terminate', 'next_values_out'):
        assert refused(call(**{k: None}), b'partial next_values group'), k
    assert refused(call(rewards=None), b'partial rewards group')
    assert refused(call(rewards=None, rewards_out=None), b'accumulators need rewards')
    assert refused(call(**dict(none, rewards_out=None)), b'partial rewards group')                # rewards without a consumer
    assert refused(call(max_size=0), b'max_size') and refused(call(max_size=-1), b'max_size')
    assert refused(call(workspace_doubles=L.rollout_store_ws(16) - 1), b'workspace')
    for k in ('rewards_ss', 'dones_ss', 'next_values_ss'):
        assert refused(call(**{k: 15}), b'slot stride'), k
    assert L.rollout_store_ws(1) == 3 and L.rollout_store_ws(8) == 3 and L.rollout_store_ws(9) == 6 and L.rollout_store_ws(4096) == 1536


def test_torch_op_is_registered():
    import ase_amd.ops  # noqa: F401
    schema = str(torch.ops.ase_hip.rollout_store.default._schema)
    for name in ('rewards_out', 'dones_out', 'next_values_out', 'cur_rewards', 'cur_lengths', 'meter', 'done_ids_out'):
        assert f'!)? {name}' in schema, (name, schema)
    assert '!)[] dsts' in schema and 'Tensor? slot_dev=None' in schema and schema.endswith('-> ()')
    assert 'rollout_store(' in ase_amd.ops.__doc__
    with pytest.raises(NotImplementedError):                               # no CPU kernel: the product has no fallback
        torch.ops.ase_hip.rollout_store(torch.zeros(4, dtype=torch.uint8), 0, 1, [], [], None, 0.0, 1.0, None, None, None, None, None,
                                        None, None, None, 0, None)


# ---- the agents on the stand-in -----------------------------------------------------------------------------------------------
class _Replay:
    """A stub environment that replays recorded ``step`` returns, so that the default loop and the device loop see the same
    data: resets draw nothing (they clear progress_buf only), by index list or by mask."""
    resets_done_on_device = True

    def __init__(self, env, records):
        self._e, self._records, self._pos = env, records, 0
        self.env = self.task = self
        self.num_envs, self.viewer = env.num_envs, None
        self.observation_space, self.action_space = env.observation_space, env.action_space
        self.amp_observation_space = env.amp_observation_space
        self.progress_buf = torch.zeros(env.num_envs, dtype=torch.int32)
        self._obs = env._obs.clone()
        self.reset_calls, self.reset_done_calls = 0, 0

    def get_task_obs_size(self):
        return 0

    def fetch_amp_obs_demo(self, n):
        return self._e.fetch_amp_obs_demo(n)

    def reset(self, env_ids=None):
        self.reset_calls += 1
        if env_ids is None:
            self.progress_buf.zero_()
        elif len(env_ids) > 0:
            self.progress_buf[torch.as_tensor(env_ids, dtype=torch.long).view(-1)] = 0
        return self._obs.clone()

    def reset_done(self, mask):
        self.reset_done_calls += 1
        self.progress_buf.mul_((mask.view(-1) == 0).to(torch.int32))
        return self._obs.clone()

    def step(self, actions):
        obs, rewards, dones, infos = self._records[self._pos]
        self._pos += 1
        self.progress_buf += 1
        self._obs = obs.clone()
        return obs.clone(), rewards.clone(), dones.clone(), {k: v.clone() for k, v in infos.items()}


def _records(G, steps):
    env = T._env(G, seed=9)
    recs = [env.step(None) for _ in range(steps)]
    return recs


def _raiser(name):
    def f(*a, **kw):
        raise AssertionError(f'{name} called on the device_rollout path')
    return f


@pytest.mark.parametrize('kind', ('amp', 'ase'))
def test_agent_device_rollout_equals_the_default_path(kind, golden_dir, monkeypatch):
    G = T._load(golden_dir, kind)
    H = G['cfg']['horizon_length']
    recs = _records(G, H)
    assert sum(int(r[2].sum()) for r in recs) > 0
    extra = dict(device_latents=True) if kind == 'ase' else {}
    env_h, env_d = _Replay(T._env(G), recs), _Replay(T._env(G), recs)
    host, _ = T._agent(G, env_h, be=EmuRolloutStore(), **extra)
    dev, _ = T._agent(G, env_d, be=EmuRolloutStore(), device_rollout=True, **extra)
    assert isinstance(dev.game_rewards, agents.DeviceMeter) and isinstance(host.game_rewards, agents.AverageMeter)
    dev.set_weights(host.get_weights())                                # one initialisation for both
    host.play_steps()
    assert host.backend.store_calls == 0 and env_h.reset_done_calls == 0
    monkeypatch.setattr(torch.Tensor, 'nonzero', _raiser('Tensor.nonzero'))
    monkeypatch.setattr(torch, 'any', _raiser('torch.any'))
    monkeypatch.setattr(agents.AverageMeter, 'update', _raiser('AverageMeter.update'))
    dev.play_steps()
    monkeypatch.undo()
    assert dev.backend.store_calls == H and env_d.reset_done_calls == H and env_d.reset_calls == 1
    assert set(dev.experience) == set(host.experience)
    for k in host.experience:
        R.same(dev.experience[k], host.experience[k], f'{kind} experience {k}')
    R.same(dev.current_rewards, host.current_rewards, 'current_rewards')
    R.same(dev.current_lengths, host.current_lengths, 'current_lengths')
    if kind == 'ase':
        R.same(dev._ase_latents, host._ase_latents, 'latents')
        assert dev.engine.rng_state.tolist() == host.engine.rng_state.tolist()
        assert torch.equal(dev._latent_reset_steps, host._latent_reset_steps)
    # the meters: the f64 restatement over the recorded steps, the host's f32 meters as the anchor
    N = env_h.num_envs
    cr, cl, words = torch.zeros(N, 1), torch.zeros(N), [0.0, 0.0, 0.0, 0.0]
    for obs, rewards, dones, infos in recs:
        ref = R.ref_step(rewards.view(N, 1), dones, infos['terminate'], torch.zeros(N, 1), cr, cl, 0.0, 1.0)
        cr, cl = ref['cur_rewards'], ref['cur_lengths']
        words = R.meter_words(words, ref['pushed_r'], ref['pushed_l'], dev.games_to_track)
    got = dev._meter_words.tolist()
    assert got[2] == words[2] == host.game_rewards.current_size == dev.game_rewards.current_size and got[3] == words[3] > 0
    for i, m in ((0, host.game_rewards), (1, host.game_lengths)):
        a = float(m.mean.double())
        assert abs(got[i] - a) <= 2.0 * abs(a - words[i]) + 2.0 ** -23 * abs(words[i]), (i, got[i], a, words[i])
    first = lambda x: float(x.reshape(-1)[0])
    assert abs(first(dev.game_rewards.get_mean()) - first(host.game_rewards.get_mean())) <= 1e-5 * abs(words[0])
    dev.game_rewards.clear()
    assert dev.game_lengths.current_size == 0 and float(dev.game_rewards.get_mean()) == 0.0


@pytest.mark.parametrize('kind', ('ppo', 'amp', 'ase'))
def test_default_path_never_touches_the_entry(kind, golden_dir):
    class Refusing(EmuBackend):
        def rollout_store(self, *a, **kw):
            raise AssertionError('rollout_store called without device_rollout')
    G = T._load(golden_dir, kind)
    ag, _ = T._agent(G, T._env(G), be=Refusing())
    assert ag._device_rollout is False and isinstance(ag.game_rewards, agents.AverageMeter)
    ag.play_steps()
    assert not hasattr(ag, '_meter_words') and not hasattr(ag, '_done_ids')


def test_train_loop_with_the_key(golden_dir, tmp_path):
    """agent.train() with device_rollout on SyntheticVecEnv.reset_done: epochs to the end, meters read once per epoch."""
    G = T._load(golden_dir, 'amp')
    env = T._env(G)
    ag, _ = T._agent(G, env, be=EmuRolloutStore(), device_rollout=True, max_epochs=2, train_dir=str(tmp_path), name='run')
    ag.train()
    assert ag.backend.store_calls == 3 * ag.horizon_length and ag.game_rewards.current_size > 0
    assert 'rewards0/frame' in ag.writer.scalars and ag.game_lengths.get_mean() > 0
    assert int(ag._meter_words[3]) >= ag.game_rewards.current_size


class _Without:
    """An environment of before: everything of the stand-in but ``resets_done_on_device``."""

    def __init__(self, env):
        self._e = env

    def __getattr__(self, k):
        if k == 'resets_done_on_device':
            raise AttributeError(k)
        v = getattr(self._e, k)
        return self if v is self._e else v


class _ForeignObserver(agents._NullObserver):
    pass


class _IdObserver(agents._NullObserver):
    accepts_done_ids = True

    def __init__(self):
        self.lists = []

    def process_infos(self, infos, done_indices):
        self.lists.append(done_indices.clone())


def test_key_refusals(golden_dir):
    G = T._load(golden_dir, 'amp')
    be = EmuRolloutStore
    with pytest.raises(AssertionError, match='resets_done_on_device'):
        T._agent(G, _Without(T._env(G)), be=be(), device_rollout=True)
    ag, _ = T._agent(G, _Without(T._env(G)), be=be())                  # without the key such an environment still does
    assert ag._device_rollout is False
    GA = T._load(golden_dir, 'ase')
    with pytest.raises(AssertionError, match='device_latents'):
        T._agent(GA, T._env(GA), be=be(), device_rollout=True)
    env = T._env(G)
    info = {'observation_space': env.observation_space, 'action_space': env.action_space,
            'amp_observation_space': env.amp_observation_space, 'agents': 2}
    with pytest.raises(AssertionError, match='num_agents == 1'):
        T._agent(G, env, be=be(), device_rollout=True, env_info=info, minibatch_size=2 * G['cfg']['minibatch_size'])
    with pytest.raises(AssertionError, match='accepts_done_ids'):
        T._agent(G, T._env(G), be=be(), device_rollout=True, features={'observer': _ForeignObserver()})
    with pytest.raises(AssertionError, match='rollout_store'):
        T._agent(G, T._env(G), be=EmuBackend(), device_rollout=True)
    obs = _IdObserver()
    ag, _ = T._agent(G, T._env(G), be=be(), device_rollout=True, features={'observer': obs})
    ag.play_steps()
    assert len(obs.lists) == ag.horizon_length
    for n, ids in enumerate(obs.lists):                                # the device list of each step: e where done, else -1
        done = ag.experience['dones'][n] != 0
        rows = torch.arange(ids.numel(), dtype=torch.int32)
        assert ids.dtype == torch.int32 and torch.equal(ids, torch.where(done, rows, torch.full_like(rows, -1)))


def test_hrl_agent_with_the_key(golden_dir, tmp_path, monkeypatch):
    """HRLAgent.env_step hands float dones and a float terminate to the store; disc_rewards is a row of the field table."""
    cfg, env, llc, GL, GH = T._hrl_setup(golden_dir, tmp_path)
    cfg.update(backend=EmuRolloutStore(), device_rollout=True)
    ag = agents.HRLAgent('hrl', cfg)
    seen = []
    step = ag.env_step

    def recording_step(actions):
        out = step(actions)
        seen.append((out[2].clone(), out[3]['terminate'].clone(), out[3]['disc_rewards'].clone(), out[1].clone()))
        return out
    ag.env_step = recording_step
    monkeypatch.setattr(torch.Tensor, 'nonzero', _raiser('Tensor.nonzero'))
    ag.play_steps()
    monkeypatch.undo()
    E = ag.experience
    assert len(seen) == ag.horizon_length == ag.backend.store_calls and seen[0][0].dtype == torch.float32
    for n, (dones, terminate, disc, rewards) in enumerate(seen):
        R.same(E['dones'][n], (dones != 0).to(torch.uint8), f'hrl dones {n}')
        R.same(E['disc_rewards'][n], disc.view(-1, 1), f'hrl disc_rewards {n}')
        R.same(E['rewards'][n], (rewards + ag._reward_shift) * ag._reward_scale, f'hrl rewards {n}')
    total = sum(int((s[0] != 0).sum()) for s in seen)
    assert total > 0 and int(ag._meter_words[3]) == total and ag.game_rewards.current_size == min(total, ag.games_to_track)


def test_host_addresses_never_reach_the_launch():
    """HipBackend.rollout_store takes raw addresses: a tensor that is not on the backend's GPU is refused by an assertion
    before the table is built or the library is called (here: a backend object without a GPU behind it, so nothing can run)."""
    from ase_amd.backend import HipBackend
    be = object.__new__(HipBackend)
    be.device = torch.device('cuda:0')
    n = 8
    with pytest.raises(AssertionError, match='dones: a tensor on cuda:0'):
        be.rollout_store(torch.zeros(n, dtype=torch.uint8))
    with pytest.raises(AssertionError, match='fields: tensors on cuda:0'):
        be._rollout_store_table(n, 2, [(torch.zeros(n, 3), torch.zeros(2, n, 3))])
    for who, dtype in (('rewards', torch.float32), ('terminate', None), ('done_ids_out', torch.int32)):
        with pytest.raises(AssertionError, match=f'{who}: a tensor on cuda:0'):
            be._rs_vec(torch.zeros(n, dtype=dtype or torch.uint8), n, dtype, who)
    assert not be._here(torch.zeros(1))


def test_meters_are_read_once_per_rollout(golden_dir):
    """current_size and the two get_mean() of train() share one fetch of the four words; the next rollout drops it."""
    G = T._load(golden_dir, 'amp')
    ag, _ = T._agent(G, T._env(G), be=EmuRolloutStore(), device_rollout=True)

    class Counting:
        def __init__(self, t):
            self.t, self.reads = t, 0

        def cpu(self):
            self.reads += 1
            return self.t.cpu()

        def __getitem__(self, k):
            return self.t[k]
    ag.play_steps()
    words = ag._meter_host.words = Counting(ag._meter_words)
    size, mean_r, mean_l = ag.game_rewards.current_size, ag.game_rewards.get_mean(), ag.game_lengths.get_mean()
    assert words.reads == 1 and size == int(ag._meter_words[2]) > 0
    assert float(mean_r) == float(ag._meter_words[0].float()) and float(mean_l) == float(ag._meter_words[1].float())
    ag.play_steps()
    assert ag.game_rewards.current_size == int(ag._meter_words[2]) and words.reads == 2
    ag.game_lengths.clear()
    assert ag.game_rewards.current_size == 0 and words.reads == 3 and not ag._meter_words[:3].any()
