"""CPU stand-in of ``HipBackend.rollout_store``, on top of the op emulator: the contract of
``ase_hip_rollout_store`` (include/ase_hip.h) row by row in torch - selections instead of index lists, f32 where the kernel
computes in f32, the meters in f64 - with the entry's refusals as assertions.  TEST INFRASTRUCTURE ONLY: it lets the agents'
``device_rollout`` run without a GPU; the reference it is checked against is tests/ref_rollout_store.py."""
import torch

from ase_amd import lib as L
from tests.test_latent_renew_emu import EmuWithLatents

_KINDS = (torch.uint8, torch.bool, torch.int32, torch.int64, torch.float32)


class EmuRolloutStore(EmuWithLatents):
    name = "emu-rollout-store"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.store_calls = 0

    def rollout_store(self, dones, slot=0, n_slots=None, fields=(), rewards=None, shift=0.0, scale=1.0, rewards_out=None,
                      dones_out=None, next_values=None, terminate=None, next_values_out=None, cur_rewards=None,
                      cur_lengths=None, meter=None, max_size=0, workspace=None, done_ids_out=None, slot_dev=None):
        self.store_calls += 1
        n = dones.numel()
        f32 = torch.float32
        acc = (cur_rewards, cur_lengths, meter)
        assert n > 0 and len(fields) <= L.ROLLOUT_STORE_MAX_FIELDS and dones.dtype in _KINDS
        assert all(t is None for t in acc) or all(t is not None for t in acc), 'partial accumulator group'
        nv = (next_values, terminate, next_values_out)
        assert all(t is None for t in nv) or all(t is not None for t in nv), 'partial next_values group'
        assert terminate is None or terminate.dtype in _KINDS
        assert (rewards is not None) == (rewards_out is not None or meter is not None), 'partial rewards group'
        assert meter is None or max_size > 0
        for t in (rewards_out, dones_out, next_values_out):
            if t is not None:
                assert n_slots in (None, t.shape[0])
                n_slots = t.shape[0]
        if n_slots is None:
            n_slots = fields[0][1].shape[0] if fields else 1
        assert 0 <= slot < n_slots
        if slot_dev is not None:
            slot = int(slot_dev)
            if not 0 <= slot < n_slots:
                return                                             # a slot word outside the buffer: nothing is written
        flags = dones.reshape(-1)
        done, d = flags != 0, flags.to(f32)
        for src, dst in fields:
            dst[slot].view(n, -1).copy_(src.reshape(n, -1))
        if rewards_out is not None:
            rewards_out[slot].view(-1).copy_((rewards.reshape(-1) + torch.tensor(shift, dtype=f32)) * torch.tensor(scale, dtype=f32))
        if dones_out is not None:
            dones_out[slot].view(-1).copy_(done.to(torch.uint8))
        if next_values_out is not None:
            next_values_out[slot].view(-1).copy_(next_values.reshape(-1) * (1.0 - terminate.reshape(-1).to(f32)))
        if done_ids_out is not None:
            rows = torch.arange(n, dtype=torch.int32)
            done_ids_out.view(-1).copy_(torch.where(done, rows, torch.full_like(rows, -1)))
        if meter is None:
            return
        r = cur_rewards.reshape(-1) + rewards.reshape(-1)
        l = cur_lengths.reshape(-1) + 1.0
        k = int(done.sum())
        if k > 0:
            zero = torch.zeros(n, dtype=torch.float64)
            sums = [float(torch.where(done, x.double(), zero).sum()) for x in (r, l)]
            size = min(k, int(max_size))
            old = min(int(max_size) - size, int(meter[2]))
            for i in (0, 1):
                meter[i] = (float(meter[i]) * old + (sums[i] / k) * size) / (old + size)
            meter[2] = old + size
            meter[3] += k
        keep = 1.0 - d
        cur_rewards.view(-1).copy_(r * keep)
        cur_lengths.view(-1).copy_(l * keep)
