"""CPU stand-in of ``HipBackend.hrl_latent / hrl_llc_action / hrl_accum``, on top of the op emulator: the
contracts of the three entries (include/ase_hip.h) in torch, one f32 operation per statement, with the entries' refusals as
assertions.  TEST INFRASTRUCTURE ONLY: it lets the agents' ``device_llc_step`` run without a GPU; the reference it is checked
against is tests/ref_hrl_step.py."""
import torch

from tests.emu_rollout_store import EmuRolloutStore

_KINDS = (torch.uint8, torch.bool, torch.int32, torch.int64, torch.float32)
_STORAGE = (torch.float32, torch.bfloat16, torch.float16)


def _clamp(x):
    """torch.clamp(x, -1, 1) as floor_nan / ceil_nan have it: selections, so a NaN stays NaN and -0.0 stays -0.0."""
    one = torch.ones((), dtype=x.dtype)
    x = torch.where(x < -one, -one, x)
    return torch.where(x > one, one, x)


class EmuHrlStep(EmuRolloutStore):
    name = "emu-hrl-step"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.hrl_calls = {'latent': 0, 'llc_action': 0, 'accum': 0}

    def hrl_latent(self, actions, z=None, z2=None, dim=None):
        self.hrl_calls['latent'] += 1
        n = actions.shape[0]
        dim = actions.shape[1] if dim is None else int(dim)
        assert actions.dtype == torch.float32 and (z is not None or z2 is not None)
        assert 1 <= dim <= 128 and actions.shape[1] >= dim and n >= 1
        assert z is None or (z.dtype == torch.float32 and z.shape[0] == n and z.shape[1] >= dim)
        assert z2 is None or (z2.dtype in _STORAGE and z2.shape[0] == n and z2.shape[1] >= dim)
        out = torch.empty(n, dim, dtype=torch.float32)
        self.normalize_rows(_clamp(actions[:, :dim]), out, n, dim)          # the row code normalize_rows runs
        if z is not None:
            z[:, :dim] = out
        if z2 is not None:
            self.gather_rows(out, dim, None, (0, 0), n, z2)                 # latent_store_as: gather_rows' conversion

    def hrl_llc_action(self, mu, low, high, out, act, clip=True):
        self.hrl_calls['llc_action'] += 1
        n, act = mu.shape[0], int(act)
        assert mu.dtype == torch.float32 and out.dtype == torch.float32 and 1 <= act <= 128 and n >= 1
        assert mu.shape[1] >= act and out.shape[0] == n and out.shape[1] >= act
        m = mu[:, :act]
        if clip:
            assert low.numel() == act and high.numel() == act
            d = (high - low) / 2.0
            c = (high + low) / 2.0
            p = _clamp(m) * d
            m = p + c
        out[:, :act] = m

    def hrl_accum(self, rewards, dones, acc, first, last, llc_steps, terminate=None, logit=None, disc_scale=1.0, rewards_out=None,
                  disc_out=None, dones_out=None, terminate_out=None):
        self.hrl_calls['accum'] += 1
        n, f32 = dones.numel(), torch.float32
        assert n >= 1 and rewards.dtype == f32 and rewards.numel() == n and dones.dtype in _KINDS
        assert terminate is None or (terminate.dtype in _KINDS and terminate.numel() == n)
        assert acc.dtype == f32 and acc.shape == (4, n) and llc_steps >= 1
        assert terminate is not None or terminate_out is None, 'partial terminate group'
        assert logit is not None or disc_out is None, 'partial discriminator group'
        assert not last or (rewards_out is not None and dones_out is not None), 'last without rewards_out / dones_out'
        assert not last or terminate is None or terminate_out is not None, 'partial terminate group'
        assert not last or logit is None or disc_out is not None, 'partial discriminator group'
        zero = torch.zeros(n, dtype=f32)

        def fold(row, x):
            s = (zero if first else acc[row]) + x.reshape(-1).to(f32)
            acc[row] = s
            return s
        r = fold(0, rewards)
        d = fold(2, dones)
        dr = t = None
        if logit is not None:
            x = torch.empty(n, 1, dtype=f32)
            self.disc_reward(logit, x, n, disc_scale)
            dr = fold(1, x)
        if terminate is not None:
            t = fold(3, terminate)
        if not last:
            return
        steps = torch.tensor(float(llc_steps), dtype=f32)
        rewards_out.view(-1).copy_(r / steps)
        dones_out.view(-1).copy_((d > 0).to(f32))
        if dr is not None:
            disc_out.view(-1).copy_(dr / steps)
        if t is not None:
            terminate_out.view(-1).copy_((t > 0).to(f32))
