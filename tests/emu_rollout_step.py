"""CPU stand-in of ``HipBackend.rollout_head`` / ``word_step`` and of the library's launch programs, on top
of the op emulator: the contract of ``ase_hip_rollout_head`` (include/ase_hip.h) in the expressions the emulator already uses
for ``rms_normalize`` and ``gather_rows``, with the entry's refusals as assertions.  TEST INFRASTRUCTURE ONLY: it lets the
agents' ``rollout_program`` run without a GPU; the reference it is checked against is tests/ref_rollout_step.py.

Programs: between ``prog_begin`` and ``prog_end`` every backend call and every ``host_call`` is kept as a closure and NOTHING
runs - a caller that reads a result while it records reads stale memory, as on the device; ``prog_launch`` runs the closures in
order."""
import torch

from tests.emu_backend import _store
from tests.emu_rollout_store import EmuRolloutStore

_PASS = ('prog_create', 'prog_begin', 'prog_end', 'prog_launch', 'prog_size', 'prog_destroy', 'host_call')


class EmuRolloutStep(EmuRolloutStore):
    name = "emu-rollout-step"
    _rec, _depth, calls = None, 0, ()

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._progs, self._rec = {}, None
        self.calls = []                      # names of the backend calls made (eagerly or into a recording), in order
        self.prog_begins = 0

    # ---- launch programs -----------------------------------------------------------------------------------------------------
    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith('_') or name in _PASS or not callable(v) or isinstance(v, type):
            return v
        calls, rec = object.__getattribute__(self, 'calls'), object.__getattribute__(self, '_rec')
        if object.__getattribute__(self, '_depth') > 0 or isinstance(calls, tuple):          # a call from inside a call: not counted
            return v

        def call(*a, **kw):
            calls.append(name)
            if rec is not None:
                rec.append(lambda: v(*a, **kw))
                return None
            self._depth += 1
            try:
                return v(*a, **kw)
            finally:
                self._depth -= 1
        return call

    def prog_create(self):
        key = len(self._progs) + 1
        self._progs[key] = []
        return key

    def prog_begin(self, prog):
        assert self._rec is None, 'a program is already recording'
        self.prog_begins += 1
        self._progs[prog] = []
        self._rec = self._progs[prog]

    def prog_end(self, prog):
        assert self._rec is self._progs[prog]
        self._rec = None

    def host_call(self, fn):
        if self._rec is None:
            fn()
        else:
            self._rec.append(fn)

    def prog_launch(self, prog):
        assert self._rec is None, 'a replay inside a recording'
        self._depth += 1                                               # (what a closure calls inside itself is not counted)
        try:
            for fn in self._progs[prog]:
                fn()
        finally:
            self._depth -= 1

    def prog_size(self, prog):
        return len(self._progs[prog])

    def prog_destroy(self, prog):
        self._progs.pop(prog, None)

    # ---- the two entries -----------------------------------------------------------------------------------------------------
    def rollout_head(self, obs, z=None, mean=None, std=None, xa=None, xc=None, zc=None, zs=None, obses_out=None, z_out=None,
                     slot=0, slot_dev=None):
        outs = (xa, xc, zc, zs, obses_out, z_out)
        assert any(t is not None for t in outs), 'no output at all'
        n, D = obs.shape
        Z = 0 if z is None else z.shape[1]
        assert n > 0 and D > 0 and obs.dtype == torch.float32
        assert Z > 0 or (zc is None and zs is None and z_out is None), 'a latent output with Z == 0'
        assert (xa is None and xc is None) or (mean is not None and std is not None), 'xa / xc without mean and std'
        for t, w in ((xa, D), (xc, D), (zc, Z), (zs, Z)):
            assert t is None or (t.shape[0] == n and t.shape[1] >= w)
        if obses_out is not None or z_out is not None:
            n_slots = (obses_out if obses_out is not None else z_out).shape[0]
            assert 0 <= slot < n_slots
            if slot_dev is not None:
                slot = int(slot_dev)
                if not 0 <= slot < n_slots:
                    return                                         # a slot word outside the buffer: nothing is written
        if xa is not None or xc is not None:
            y = torch.clamp((obs - mean[:D]) / std[:D], -5.0, 5.0)       # EmuBackend.rms_normalize's expression
            for o in (xa, xc):
                if o is not None:
                    o[:, :D] = y.to(o.dtype)
        for o in (zc, zs):
            if o is not None:
                o[:, :Z] = _store(z, o.dtype)                      # EmuBackend.gather_rows's conversion
        if obses_out is not None:
            obses_out[slot].view(torch.int32).copy_(obs.view(torch.int32))
        if z_out is not None:
            z_out[slot].view(torch.int32).copy_(z.view(torch.int32))

    def word_step(self, word, add=1, wrap=0):
        assert word.dtype == torch.int32 and word.numel() == 1
        v = int(word) + int(add)
        if wrap > 0:
            v %= int(wrap)
        v = (v + 2 ** 31) % 2 ** 32 - 2 ** 31                      # the low 32 bits, two's complement
        word.fill_(v)
