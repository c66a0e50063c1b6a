"""ForwardEngine (ase_amd/forward.py) against the UpdateEngine that derives from it, on CPU with the op emulator: a forward-only
engine and a trainer bound to the same network issue the same backend calls on operands of the same shapes and return the same
bits from policy_forward / policy_act / amp_heads - and the forward-only engine carries no training state."""
import os

import pytest
import torch

from ase_amd.engine import UpdateEngine
from ase_amd.forward import ForwardEngine
from tests.emu_backend import EmuBackend
from tests.emu_learned_sigma import LearnedSigmaEmu
from tests.helpers import build_net, set_rms

CASES = ['ase_tiny', 'ase_sep_tiny', 'amp_tiny', 'ppo_tiny', 'ase_sighead_tiny']
ROWS = (5, 67, 5)            # scratch growth (5 -> 67) and reuse of a slice of the grown buffers (67 -> 5)
TRAINING_STATE = ('grads', 'adam_m', 'adam_v', 'opt_state', 'acc', 'scaler', 'res_ring')


class Recorder:
    """Thin wrapper of a backend: every method call is noted as (name, shapes and dtypes of its tensor arguments)."""

    def __init__(self, be):
        self._be, self.calls = be, []

    @staticmethod
    def _tensors(x):
        if torch.is_tensor(x):
            yield tuple(x.shape), x.dtype
        elif isinstance(x, (list, tuple)):
            for y in x:
                yield from Recorder._tensors(y)
        elif isinstance(x, dict):
            for k in sorted(x):
                yield from Recorder._tensors(x[k])

    def __getattr__(self, name):
        v = getattr(self._be, name)
        if not callable(v):
            return v

        def call(*a, **kw):
            self.calls.append((name, tuple(self._tensors(a)) + tuple(self._tensors(kw))))
            return v(*a, **kw)
        return call


def engine_pair(G, make_be, dtype, device='cpu'):
    """(forward-only engine, trainer) on ONE network, the same running statistics in both."""
    kind, cfg, E = G['kind'], dict(G['cfg']), G['epochs'][0]
    assert cfg['normalize_value']           # (the value un-normalisation launch is part of what is compared)
    net = build_net(G, device)
    M = cfg['minibatch_size']
    amb = cfg.get('amp_minibatch_size', 0) if kind != 'ppo' else 0
    fwd = ForwardEngine(kind, net, cfg, Recorder(make_be()), dtype=dtype)
    upd = UpdateEngine(kind, net, cfg, Recorder(make_be()), minibatch=M, amp_minibatch=amb, dtype=dtype)
    for e in (fwd, upd):
        set_rms(e.obs_state, E['rms_step0_before']['obs'])
        if kind != 'ppo':
            set_rms(e.amp_state, E['rms_step0_before']['amp'])
        e.val_state.copy_(torch.tensor([0.25, 2.0, 10.0], dtype=torch.float64))
    return fwd, upd


def _both(fwd, upd, call):
    """Run `call(engine)` on both engines; the recorded backend calls must agree.  Returns the two results."""
    out = []
    for e in (fwd, upd):
        e.be.calls.clear()
        out.append(call(e))
    assert fwd.be.calls and fwd.be.calls == upd.be.calls
    return out


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), what


def compare_engines(G, make_be, dtype, device='cpu'):
    fwd, upd = engine_pair(G, make_be, dtype, device)
    kind = G['kind']
    assert type(fwd) is ForwardEngine and isinstance(upd, ForwardEngine)
    for name in TRAINING_STATE:
        assert not hasattr(fwd, name) and hasattr(upd, name), name
    if kind == 'ase':
        assert fwd.rng_state.shape == (2,) and torch.equal(fwd.rng_state, upd.rng_state)
    g = torch.Generator().manual_seed(11)
    for n in ROWS:
        obs = (torch.randn(n, fwd.obs, generator=g) * 2.0).to(device)
        z = None
        if kind == 'ase':
            z = torch.nn.functional.normalize(torch.randn(n, fwd.z, generator=g), dim=-1).to(device)
        a, b = _both(fwd, upd, lambda e: e.policy_forward(obs, z, want=('mu', 'value', 'logstd')))
        for k in ('mu', 'value', 'logstd'):
            _same(a[k], b[k], ('policy_forward', k, n))
        probs = None
        if kind != 'ppo':
            probs = torch.zeros(n, device=device)
            probs[: n // 2] = 1.0
        rngs = [torch.tensor([77, 3], dtype=torch.int64, device=device) for _ in range(2)]
        it = iter(rngs)
        a, b = _both(fwd, upd, lambda e: e.policy_act(obs, z, probs, next(it)))
        assert set(a) == set(b)
        for k in a:
            if a[k] is None:
                assert b[k] is None, k
            else:
                _same(a[k], b[k], ('policy_act', k, n))
        assert torch.equal(rngs[0], rngs[1]) and int(rngs[0][1]) != 3           # both advanced, to the same position
        if kind != 'ppo':
            amp = (torch.randn(n, fwd.amp, generator=g) * 2.0).to(device)
            (hd_a, enc_a), (hd_b, enc_b) = _both(fwd, upd, lambda e: e.amp_heads(amp))
            _same(hd_a, hd_b, ('amp_heads logits', n))
            if kind == 'ase':
                _same(enc_a, enc_b, ('amp_heads encoder', n))
            else:
                assert enc_a is None and enc_b is None


@pytest.mark.parametrize('name', CASES)
def test_forward_engine_equals_update_engine(name, golden_dir):
    G = torch.load(os.path.join(golden_dir, name + '.pt'), weights_only=False)
    compare_engines(G, LearnedSigmaEmu if 'sighead' in name else EmuBackend, torch.float32)


def test_restored_player_runs_a_forward_engine(golden_dir, tmp_path):
    """The values a restored player reaches are tests/test_boundary_emu.py's; here: it reaches them without a trainer."""
    import tests.test_boundary_emu as T
    from ase_amd.learning import players
    G = T._load(golden_dir, 'ase')
    ag, cfg = T._agent(G, T._env(G))
    ag.save(os.path.join(str(tmp_path), 'p'))
    pcfg = dict(cfg)
    pcfg.update(vec_env=T._env(G, seed=9), env_info=None, backend=EmuBackend(), player={'games_num': 1, 'print_stats': False})
    pl = players.ASEPlayer(pcfg)
    pl.restore(os.path.join(str(tmp_path), 'p.pth'))
    assert isinstance(pl.engine, ForwardEngine) and not isinstance(pl.engine, UpdateEngine)
    assert pl.model.a2c_network.infer.eng is pl.engine
    assert isinstance(ag.engine, UpdateEngine)
