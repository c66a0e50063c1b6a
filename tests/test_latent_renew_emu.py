"""Renewals of the ASE latents without a GPU: the restatement tests/emu_latent_renew.py against the recording of
the reference's own ``env_reset`` / ``_update_latents`` (tests/golden/latent_renew.pt), the conditions the generator of that
file promises, the device draws against the stream's specification (tests/ref_rollout.py), the integer reduction of the step
counts against its definition, the host-side operand checks of ``ase_hip_latent_renew``, and ``ASEAgent`` with
``device_latents`` on a stand-in backend."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from ase_amd import lib as L
from tests import emu_latent_renew as E
from tests import ref_rollout as RR
from tests import test_boundary_emu as T
from tests.emu_backend import EmuBackend

SEED = (1 << 33) + 12345


@pytest.fixture(scope='module')
def G():
    return E.load_fixture()


# ---- the restatement against the recording ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E.SCENARIOS)
def test_restatement_reproduces_the_reference_bitwise(G, name):
    """f32, whole tensors: the renewed rows as the reference wrote them, every other row the patterned prefill."""
    sc = G['scenarios'][name]
    latents, reset_steps = E.expected(G, name, torch.float32)
    assert latents.dtype == torch.float32 and torch.equal(latents, sc['latents'])
    assert reset_steps.dtype == torch.int32 and torch.equal(reset_steps, sc['reset_steps'])


def test_update_scenario_in_due_mode_finds_the_recorded_rows(G):
    """Due mode of the restatement selects exactly the recorded due list: the <= test with the steps on the left."""
    sc = G['scenarios']['update']
    latents, reset_steps, progress = E.prefill(G, 'update')
    z2 = torch.full((G['num_envs'], G['dim']), -7.0)
    rng = torch.tensor([SEED, 3], dtype=torch.int64)
    E.EmuLatentRenew().latent_renew(latents, rng_state=rng, progress_buf=progress, reset_steps=reset_steps, steps_add=True,
                                    steps_low=G['steps_low'], steps_high=G['steps_high'], z2=z2)
    lat0, steps0, _ = E.prefill(G, 'update')
    changed = (latents != lat0).any(dim=-1).nonzero().flatten().tolist()
    assert changed == sorted(sc['env_ids']) == (reset_steps != steps0).nonzero().flatten().tolist()
    assert torch.equal(z2, latents) and rng.tolist() == [SEED, 4] and torch.equal(progress, sc['progress_buf'])


# ---- the generator's promises, re-checked on the committed file ------------------------------------------------------------
def test_fixture_keeps_its_conditions(G):
    N, dim, lo, hi = G['num_envs'], G['dim'], G['steps_low'], G['steps_high']
    assert (N, dim, lo, hi) == (32, 64, 1, 150) and set(G['scenarios']) == set(E.SCENARIOS) and G['roundings'] == 16
    ids = G['scenarios']['reset_ids']['env_ids']
    assert len(ids) == 20 and len(set(ids)) == 20 and ids != sorted(ids) and all(0 <= e < N for e in ids)
    assert G['scenarios']['reset_all']['env_ids'] == list(range(N))
    up = G['scenarios']['update']
    due = (up['reset_steps0'] <= up['progress_buf']).nonzero().flatten().tolist()
    assert up['env_ids'] == due and len(due) >= 6 and N - len(due) >= 6
    assert up['progress_buf'].dtype == torch.int64 and up['reset_steps0'].dtype == torch.int32
    edge, below = G['edge_row'], G['below_row']
    assert int(up['reset_steps0'][edge]) == int(up['progress_buf'][edge]) and edge in due                 # the <= edge
    assert int(up['reset_steps0'][below]) == int(up['progress_buf'][below]) + 1 and below not in due      # one below it
    for name in E.SCENARIOS:
        sc = G['scenarios'][name]
        ids = sc['env_ids']
        others = [e for e in range(N) if e not in ids]
        assert sc['eps'].dtype == torch.float32 and sc['eps'].shape == (len(ids), dim)
        assert float(sc['eps'].norm(dim=-1).min()) >= 1.0, name
        assert sc['steps'].dtype == torch.int32 and bool(((sc['steps'] >= lo) & (sc['steps'] < hi)).all())
        # untouched rows are part of the record
        lat0, steps0, _ = E.prefill(G, name)
        assert torch.equal(sc['latents'][others], lat0[others]) and torch.equal(sc['reset_steps'][others], steps0[others])
        assert bool((sc['latents'][ids] != lat0[ids]).any(dim=-1).all()) and bool((sc['reset_steps'][ids] != steps0[ids]).all())
        assert torch.allclose(sc['latents'][ids].norm(dim=-1), torch.ones(len(ids)), atol=1e-6)
        # the allowance is the reference's own error, capped at a handful of f32 roundings of 1.0
        l64, s64 = E.expected(G, name, torch.float64)
        assert torch.equal(s64, sc['reset_steps'])
        assert float((sc['latents'][ids].double() - l64[ids]).abs().max()) == pytest.approx(sc['e_ref'], rel=1e-6, abs=1e-12)
        assert sc['e_ref'] <= G['roundings'] * 2.0 ** -24, (name, sc['e_ref'])
    assert os.path.getsize(os.path.join(E.GOLDEN, 'latent_renew.pt')) < 64 * 1024


def test_recorded_draws_come_in_call_order(G):
    """The reference draws the normals of all rows first (sample_latents), then the steps (randint_like): the recorded eps and
    steps are those two calls under the scenario's seed."""
    for name in E.SCENARIOS:
        sc = G['scenarios'][name]
        n = len(sc['env_ids'])
        torch.manual_seed(sc['seed'])
        eps = torch.normal(torch.zeros([n, G['dim']]))
        steps = torch.randint_like(torch.zeros(n, dtype=torch.int32), low=G['steps_low'], high=G['steps_high'])
        assert torch.equal(eps, sc['eps']) and torch.equal(steps, sc['steps']), name
        torch.manual_seed(sc['seed'])                                          # the other order gives other numbers
        torch.randint_like(torch.zeros(n, dtype=torch.int32), low=G['steps_low'], high=G['steps_high'])
        assert not torch.equal(torch.normal(torch.zeros([n, G['dim']])), sc['eps'])


# ---- the device draws --------------------------------------------------------------------------------------------------------
def test_step_reduction_is_exact():
    """low + ((uint64)word * (high - low) >> 32): word 0 gives low, word 0xFFFFFFFF gives high - 1 (never high), every word of
    the stream lands where floor(word / 2^32 * (high - low)) says, and the word is word 3 of element e * dim."""
    for low, high in ((1, 150), (0, 1), (-5, 3), (7, 7 + 0xFFFFFFFF)):
        assert E.reduce_steps(0, low, high) == low
        assert E.reduce_steps(0xFFFFFFFF, low, high) == high - 1
    words = RR.philox4x32_10(np.arange(2000, dtype=np.uint64), 5, SEED)[3]
    got = [E.reduce_steps(w, 1, 150) for w in words.tolist()]
    assert got == [1 + int(Fraction(w, 1 << 32) * 149) for w in words.tolist()] and min(got) == 1 and max(got) == 149
    dim, ids = 24, [0, 3, 31]
    _, steps = E.device_draws(ids, dim, SEED, 5, 1, 150)
    w3 = RR.philox4x32_10(np.asarray([e * dim for e in ids], dtype=np.uint64), 5, SEED)[3]
    assert steps.dtype == torch.int32 and steps.tolist() == [E.reduce_steps(w, 1, 150) for w in w3.tolist()]
    w0 = RR.philox4x32_10(np.asarray([e * dim for e in ids], dtype=np.uint64), 5, SEED)[0]
    assert steps.tolist() != [E.reduce_steps(w, 1, 150) for w in w0.tolist()]


@pytest.mark.parametrize('dim', (1, 63, 64, 65, 128))
def test_device_draws_are_rows_of_sample_latents(dim):
    """A renewed row e equals row e of sample_latents(n_envs, dim) at the same stream position, whichever rows are renewed."""
    n, offset = 9, (1 << 32) + 7
    ids = [7, 0, 4]
    for dt in (torch.float32, torch.float64):
        want = RR.sample_latents(n, dim, SEED, offset, dtype=dt)
        latents = torch.full((n, dim), 3.0, dtype=dt)
        rng = torch.tensor([SEED, offset], dtype=torch.int64)
        E.EmuLatentRenew().latent_renew(latents, env_ids=torch.tensor(ids + [-1, n], dtype=torch.int32), rng_state=rng)
        assert torch.equal(latents[ids], want[ids].to(dt)) and rng.tolist() == [SEED, offset + 1]
        others = [e for e in range(n) if e not in ids]
        assert bool((latents[others] == 3.0).all())
        eps, _ = E.device_draws(ids, dim, SEED, offset, dtype=dt)
        assert torch.equal(eps, RR.normals(RR.latent_elems(n, dim), offset, SEED, dt)[ids])


# ---- the C entry's operand checks ------------------------------------------------------------------------------------------
def test_entry_point_validates_operands_without_gpu():
    """The host-side checks of ase_hip_latent_renew run before any launch: refused with -1, the entry's name and the operand in
    the message."""
    lib = L.load()
    assert len(L.SIGNATURES['ase_hip_latent_renew']) == 21
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ase_hip_last_error()

    def call(mode, **kw):
        # valid calls that launch nothing: ids mode on an empty list with passed-in draws
        a = dict(env_ids=p, n_ids=0, eps=p, ld_eps=64, steps=p, rng_state=None, advance=0, progress_buf=None, progress_i64=0,
                 reset_steps=p, steps_add=0, steps_low=1, steps_high=150, latents=p, ld_z=64, z2=None, ld_z2=0, z2_dtype=L.F32,
                 n_envs=16, dim=64, stream=None)
        if mode == 'ids_rng':
            a.update(eps=None, steps=None, rng_state=p)
        elif mode == 'due':                                        # never valid without a launch: only refusals are called
            a.update(env_ids=None, eps=None, steps=None, rng_state=p, progress_buf=p, steps_add=1, z2=p, ld_z2=64)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return lib.ase_hip_latent_renew(*a.values())

    def refused(rc, *words):
        return rc == -1 and b'latent_renew' in err() and all(w in err() for w in words)

    assert call('ids') == 0 and call('ids_rng') == 0
    assert call('ids', reset_steps=None, steps=None) == 0                   # the player's resets: no steps bookkeeping
    assert call('ids', ld_z=80, ld_eps=70) == 0 and call('ids', dim=1) == 0 and call('ids', dim=128, ld_z=128, ld_eps=128) == 0
    assert refused(call('ids', latents=None), b'latents')
    assert refused(call('ids', dim=0), b'dim') and refused(call('ids', dim=129, ld_z=256, ld_eps=256), b'dim')
    assert refused(call('ids', ld_z=63), b'ld_z') and refused(call('ids', ld_eps=63), b'ld_eps')
    assert refused(call('due', ld_z2=63), b'ld_z2')
    assert refused(call('ids', n_envs=0), b'n_envs') and refused(call('ids', n_envs=-3), b'n_envs')
    assert refused(call('ids', n_ids=-1), b'n_ids') and refused(call('due', n_ids=4), b'n_ids')
    assert refused(call('ids', rng_state=p), b'one draw source', b'both')
    assert refused(call('ids', eps=None, steps=None), b'one draw source', b'none')
    assert refused(call('due', eps=p, rng_state=None, steps=p), b'eps', b'due mode')
    assert refused(call('ids_rng', steps=p), b'steps')                      # steps without eps
    assert refused(call('ids', reset_steps=None), b'steps')                 # steps without reset_steps
    assert refused(call('ids', steps=None), b'steps')                       # eps and reset_steps without steps
    assert refused(call('due', progress_buf=None), b'progress_buf', b'due mode')
    assert refused(call('due', reset_steps=None), b'reset_steps', b'due mode')
    assert refused(call('due', steps_add=0), b'steps_add', b'due mode')
    assert refused(call('ids', progress_buf=p), b'progress_buf', b'ids mode')
    assert refused(call('ids_rng', z2=p, ld_z2=64), b'z2', b'ids mode')
    assert refused(call('due', z2_dtype=7), b'z2_dtype') and refused(call('due', z2_dtype=L.F32X3), b'z2_dtype')
    for lo, hi in ((150, 150), (150, 1), (0, 1 << 32)):
        assert refused(call('ids_rng', steps_low=lo, steps_high=hi), b'steps_high'), (lo, hi)
        assert refused(call('due', steps_low=lo, steps_high=hi), b'steps_high'), (lo, hi)
    assert refused(call('ids_rng', steps_low=(1 << 31) - 4, steps_high=(1 << 31) + 4), b'int32')
    assert call('ids', steps_low=150, steps_high=1) == 0                    # passed-in steps: the range is not looked at
    assert call('ids_rng', reset_steps=None, steps_low=5, steps_high=5) == 0      # no steps drawn: neither
    with pytest.raises(L.AseHipError):
        L.check(-1, 'latent_renew')


def test_torch_op_is_registered():
    import ase_amd.ops  # noqa: F401
    assert hasattr(torch.ops.ase_hip, 'latent_renew')
    schema = str(torch.ops.ase_hip.latent_renew.default._schema)
    for name in ('latents', 'reset_steps', 'rng_state', 'z2'):
        assert f'!)? {name}' in schema or f'!) {name}' in schema, (name, schema)
    assert 'Tensor? eps,' in schema and 'Tensor? env_ids,' in schema and schema.endswith('-> ()')
    assert 'latent_renew(' in ase_amd.ops.__doc__
    with pytest.raises(NotImplementedError):                               # no CPU kernel: the product has no fallback
        torch.ops.ase_hip.latent_renew(torch.zeros(4, 8), torch.zeros(0, dtype=torch.int32), torch.zeros(0, 8), None, None, True, None,
                                       None, False, 0, 1, None)


# ---- the agent on a stand-in backend ---------------------------------------------------------------------------------------
class EmuWithLatents(EmuBackend):
    """The op emulator with the library's latent stream: sample_latents stated from tests/ref_rollout.py (the emulator's own
    draws torch.randn) and latent_renew from the restatement, so that the two paths of the agent can be compared."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.renew_calls = []

    def sample_latents(self, z, rows, dim, rng_state, row_offset=0, advance=True, z2=None):
        z[:rows, :dim] = RR.sample_latents(rows, dim, int(rng_state[0]), int(rng_state[1]), row_offset, torch.float32)
        if z2 is not None:
            z2[:rows, :dim] = z[:rows, :dim].to(z2.dtype)
        if advance:
            rng_state[1] += 1

    def latent_renew(self, latents, **kw):
        self.renew_calls.append('due' if kw.get('env_ids') is None else 'ids')
        E.EmuLatentRenew().latent_renew(latents, **kw)


def _pair(golden_dir):
    G = T._load(golden_dir, 'ase')
    env_a, env_b = T._env(G), T._env(G)
    dev, _ = T._agent(G, env_a, be=EmuWithLatents(), device_latents=True)
    host, _ = T._agent(G, env_b, be=EmuWithLatents())
    return dev, host, env_a, env_b


def test_agent_full_reset_equals_the_host_path(golden_dir):
    dev, host, _, _ = _pair(golden_dir)
    assert torch.equal(dev.engine.rng_state, host.engine.rng_state)
    pos = int(dev.engine.rng_state[1])
    dev.obs, host.obs = dev.env_reset(), host.env_reset()
    assert torch.equal(dev._ase_latents, host._ase_latents) and bool(dev._ase_latents.any())
    assert int(dev.engine.rng_state[1]) == int(host.engine.rng_state[1]) == pos + 1
    lo, hi = int(dev._latent_steps_min), int(dev._latent_steps_max)
    assert bool(((dev._latent_reset_steps >= lo) & (dev._latent_reset_steps < hi)).all())
    assert dev.backend.renew_calls == ['ids'] and host.backend.renew_calls == []


def test_agent_update_latents_on_the_device_path(golden_dir, monkeypatch):
    dev, _, env, _ = _pair(golden_dir)
    dev.obs = dev.env_reset()
    z0, steps0 = dev._ase_latents.clone(), dev._latent_reset_steps.clone()
    env.progress_buf[:] = 0
    env.progress_buf[:4] = 100
    env.progress_buf[5] = int(steps0[5])                                   # the <= edge
    env.progress_buf[6] = int(steps0[6]) - 1                               # one below it
    due = [0, 1, 2, 3, 5]
    keep = [e for e in range(env.num_envs) if e not in due]

    def no_nonzero(*a, **kw):
        raise AssertionError('nonzero called on the device path')
    monkeypatch.setattr(torch.Tensor, 'nonzero', no_nonzero)
    dev._rollout_step = 3
    dev._update_latents()
    monkeypatch.undo()
    assert torch.equal(dev._ase_latents[keep], z0[keep]) and torch.equal(dev._latent_reset_steps[keep], steps0[keep])
    assert bool((dev._ase_latents[due] != z0[due]).any(dim=-1).all())
    assert torch.allclose(dev._ase_latents[due].norm(dim=-1), torch.ones(len(due)), atol=1e-6)
    assert bool((dev._latent_reset_steps[due] > steps0[due]).all())
    slot = dev.experience['ase_latents']
    assert torch.equal(slot[3], dev._ase_latents) and not slot[2].any() and not slot[4].any()
    # _rollout_extras leaves the written slot alone (a sentinel in it survives) and copies when the launch wrote another one
    slot[3, 0, 0] = 9.0
    dev._rollout_extras(3, {'rand_action_mask': torch.ones(env.num_envs)}, {'amp_obs': dev.experience['amp_obs'][3]})
    assert float(slot[3, 0, 0]) == 9.0
    dev._rollout_extras(3, {'rand_action_mask': torch.ones(env.num_envs)}, {'amp_obs': dev.experience['amp_obs'][3]})
    assert torch.equal(slot[3], dev._ase_latents)


def test_agent_rollout_with_device_latents(golden_dir):
    """play_steps over one horizon: every slot of experience['ase_latents'] holds unit rows, written by the launches."""
    dev, _, env, _ = _pair(golden_dir)
    dev.play_steps()
    z = dev.experience['ase_latents']
    assert torch.allclose(z.norm(dim=-1), torch.ones(z.shape[:2]), atol=1e-6)
    assert dev.backend.renew_calls.count('due') == dev.horizon_length and dev._latents_slot == -1
    assert not torch.equal(z[0], z[-1])                                    # renewals happened on the way (steps in [1, 6))


def test_agent_without_the_key_never_touches_the_entry(golden_dir):
    G = T._load(golden_dir, 'ase')

    class Refusing(EmuBackend):
        def latent_renew(self, *a, **kw):
            raise AssertionError('latent_renew called without device_latents')
    ag, _ = T._agent(G, T._env(G), be=Refusing())
    assert ag._device_latents is False
    ag.play_steps()
    ag.env_reset([1, 2])
    # the plain emulator has no such entry: the default keeps working on it, the key is refused at construction
    plain, _ = T._agent(G, T._env(G))
    plain.play_steps()
    with pytest.raises(AssertionError, match='latent_renew'):
        T._agent(G, T._env(G), device_latents=True)
    with pytest.raises(AssertionError, match='latent_steps'):
        T._agent(G, T._env(G), be=EmuWithLatents(), device_latents=True, latent_steps_min=6, latent_steps_max=6)


def test_player_resets_through_the_entry(golden_dir):
    """ASEPlayer._reset_latents(ids) with device_latents: one ids-mode call without steps; other rows stay, the host-side step
    counter is untouched."""
    G = T._load(golden_dir, 'ase')
    env = T._env(G)
    ag, cfg = T._agent(G, env, be=EmuWithLatents())
    pcfg = dict(cfg)
    pcfg.update(vec_env=T._env(G, seed=4), env_info=None, backend=EmuWithLatents(), device_latents=True,
                player={'games_num': 1, 'print_stats': False})
    pl = T.PLAYERS['ase'](pcfg)
    pl._reset_latents()
    z0, count0 = pl._ase_latents.clone(), pl._latent_step_count
    pl._reset_latents([2, 5])
    changed = (pl._ase_latents != z0).any(dim=-1).nonzero().flatten().tolist()
    assert changed == [2, 5] and pl._latent_step_count == count0 and pl.backend.renew_calls == ['ids', 'ids']
    assert torch.allclose(pl._ase_latents.norm(dim=-1), torch.ones(z0.shape[0]), atol=1e-6)
