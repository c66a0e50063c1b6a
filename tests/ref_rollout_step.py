"""Reference, cases and checks of ``ase_hip_rollout_head`` / ``ase_hip_word_step``, shared by
tests/test_rollout_step_emu.py (the emulator, no GPU) and tests/test_gpu_rollout_step.py (the MI355X).

The reference is the COMPOSITION the entry replaces, in torch on the CPU - not the emulator:
  xa, xc      torch.clamp((obs - mean) / std, -5, 5) in f32 (the rms_normalize expression: IEEE subtraction, IEEE division, a
              clamp that keeps a NaN), then torch's own .to(dtype);
  zc, zs      the clamp to +-65504 followed by the cast, as tests/ref_update.py states gather_rows (``convert``: IEEE half
              saturates, a NaN is stored as F16_OF_NAN; bf16 / f32 plain);
  obses_out,  an indexed copy of the raw rows into the slot.
  z_out
torch's cast is taken on the device under test ('cpu' for the emulator, the GPU for the kernels), because torch's two casts do
not agree on the bf16 pattern of a NaN and only one of them can be met bitwise: on the machines these tests were written on,
torch's CPU cast stores 0xFFFF for every NaN (sign and payload lost), torch's GPU cast 0x7FC0 for every NaN, and the kernels
- rms_normalize, gather_rows and rollout_head alike - keep the sign and quieten: 0x7FC0 for the canonical NaN the cases carry
(0xFFC0 for a negative one, which no torch cast produces and the cases therefore do not carry).  f32 and IEEE half patterns are
the same on all three.  The f32 arithmetic in front of the cast is evaluated on the CPU either way.
Every comparison is BITWISE on integer views, over the WHOLE allocation an output is a window of: the allocations are filled
with a sentinel pattern, have wider pitches and a column offset, so every guard word - the columns at and beyond D, the pad of
every row, the other slots, the words before and behind the window - is compared after each launch.  COUNTS collects what was
looked at."""
import torch

from tests.ref_update import F16_OF_NAN, convert

F32, BF16, F16, I32 = torch.float32, torch.bfloat16, torch.float16, torch.int32
DTYPES = (F32, BF16, F16)
NS = (1, 63, 64, 65, 300)
DS = (1, 3, 4, 253, 260)
ZS = (0, 1, 64)
OUTS = ('xa', 'xc', 'zc', 'zs', 'obses_out', 'z_out')
CRITIC_ONLY = ('xc', 'zc')
COUNTS = {'launches': 0, 'elements': 0, 'guards': 0, 'vec_obs_on': 0, 'vec_obs_off': 0, 'vec_z_on': 0, 'vec_z_off': 0}
_SENT = {4: 0x5A5A5A5A, 2: 0x5A5A}
_INT = {4: torch.int32, 2: torch.int16}

# the values y = (x - mean) / std is steered to (exactly, in the columns whose mean is k / 8 and whose std is a power of two):
# NaN, +-inf, +-100 (clamped), +-5 exactly (the clamp's own bounds), the RNE ties of bf16 (1 + 2^-8: down to even, 1 + 3 2^-8: up
# to even) and of IEEE half (1 + 2^-11, 1 + 3 2^-11), their negatives, and both zeros
Y_SPECIAL = (float('nan'), float('inf'), float('-inf'), 100.0, -100.0, 5.0, -5.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11,
             1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -11), 0.0, -0.0, 4.999999523162842, -5.000000476837158)
# latents: beyond half's range on both sides, NaN, -0.0, the largest finite half, the first f32 that rounds to inf without the
# clamp, and half's RNE ties
Z_SPECIAL = (70000.0, -70000.0, float('nan'), -0.0, 65504.0, 65520.0, -65520.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8,
             float('inf'), float('-inf'))


def bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _sentinel(numel, dtype, dev='cpu'):
    es = torch.empty(0, dtype=dtype).element_size()
    return torch.full((numel,), _SENT[es], dtype=_INT[es], device=dev).view(dtype)


class Buf:
    """A strided window (shape, strides, offset in elements) of a sentinel-filled flat allocation on `dev`, with a CPU twin that
    holds what the allocation is expected to hold."""

    def __init__(self, dev, shape, strides, offset, dtype, tail=9):
        size = offset + sum((s - 1) * st for s, st in zip(shape, strides)) + 1 + tail
        self.alloc, self.want = _sentinel(size, dtype, dev), _sentinel(size, dtype)
        assert self.alloc.data_ptr() % 64 == 0, 'the allocator hands out 64-byte aligned blocks: offsets decide the alignment'
        self.view = self.alloc.as_strided(shape, strides, offset)
        self.want_view = self.want.as_strided(shape, strides, offset)
        self.window = int(torch.tensor(shape).prod())

    def put(self, values):
        """An INPUT: the same bits into the device window and the twin."""
        self.want_view.copy_(values)
        self.view.copy_(values.to(self.alloc.device))
        return self

    def check(self, what):
        got = bits(self.alloc.cpu())
        bad = got != bits(self.want)
        assert not bool(bad.any()), (what, 'words differ', int(bad.sum()), bad.nonzero()[:6].flatten().tolist(), self.alloc.numel())
        COUNTS['elements'] += self.window
        COUNTS['guards'] += self.alloc.numel() - self.window


def _steer(gen, n, W, special, mean=None, std=None):
    """Random rows with the special values in the first row, the last row and the last column; with mean / std the specials are
    targets of (x - mean) / std."""
    x = (torch.randn(n, W, generator=gen, dtype=torch.float64) * 2.5)
    sp = torch.tensor(special, dtype=torch.float64)
    m = torch.zeros(W, dtype=torch.float64) if mean is None else mean.double()
    s = torch.ones(W, dtype=torch.float64) if std is None else std.double()
    cols, rows = torch.arange(W), torch.arange(n)
    x[0] = m + sp[cols % len(sp)] * s
    x[n - 1] = m + sp[(cols + 5) % len(sp)] * s
    x[:, W - 1] = m[W - 1] + sp[(rows + 2) % len(sp)] * s[W - 1]
    return x.to(F32)


def stats(gen, D):
    """mean = k / 8, std a power of two - (x - mean) / std is exact there - but: every third column takes generic values (both
    operations round), and one column has the std of a variance of zero, sqrt(1e-5)."""
    mean = torch.randint(-16, 17, (D,), generator=gen).to(F32) / 8
    std = 2.0 ** torch.randint(-2, 2, (D,), generator=gen).to(F32)
    generic = torch.arange(D) % 3 == 1
    generic[D - 1] = False
    mean = torch.where(generic, torch.randn(D, generator=gen), mean)
    std = torch.where(generic, torch.rand(D, generator=gen) + 0.1, std)
    if D >= 3:
        std[D // 2] = torch.sqrt(torch.tensor(0.0, dtype=F32) + 1e-5)
    return mean, std


def reference(obs, z, mean, std, dtype, dev='cpu'):
    """The composition the entry replaces, on CPU tensors: (x for xa / xc, converted latents for zc / zs).  The f32 arithmetic
    runs on the CPU (IEEE, operation by operation); torch's own cast .to(dtype) runs on `dev`, the device under test - see
    the module docstring for what torch's two casts do to a NaN."""
    cast = lambda t: t.to(dev).to(dtype).cpu()
    x = cast(torch.clamp((obs - mean) / std, -5.0, 5.0))
    zz = None
    if z is not None:
        zz = cast(torch.where(torch.isnan(z), torch.full_like(z, F16_OF_NAN), z.clamp(-65504.0, 65504.0)) if dtype == F16 else z)
        assert dev != 'cpu' or torch.equal(bits(zz), bits(convert(z, dtype)))          # tests/ref_update.py's statement of gather_rows
    return x, zz


def vec_condition(obs, mean, std, xs, slotted):
    """The header's 16-bytes-per-lane condition of one side, on the launched tensors: obs [n, W]; mean / std or None; xs: the
    given x_dtype outputs; slotted: the given [n_slots, n, W] output or None."""
    W = obs.shape[1]
    ok = W % 4 == 0 and obs.stride(0) % 4 == 0 and obs.data_ptr() % 16 == 0
    if mean is not None:
        ok = ok and mean.data_ptr() % 16 == 0 and std.data_ptr() % 16 == 0
    for t in xs:
        ok = ok and t.stride(0) % 4 == 0 and t.data_ptr() % (4 * t.element_size()) == 0
    if slotted is not None:
        ok = ok and slotted.stride(1) % 4 == 0 and slotted.stride(0) % 4 == 0 and slotted.data_ptr() % 16 == 0
    return ok


class Case:
    """One launch: inputs, sentinel-filled outputs, and the expected content of every allocation.  lay: layout knobs - *_off
    (column offset of a window, elements), *_ld (pitch), ss_extra (added to a slot stride), stat_off (offset of mean / std)."""

    def __init__(self, dev, n, D, Z, dtype, outs=OUTS, n_slots=3, seed=0, **lay):
        g = torch.Generator().manual_seed(1000 * seed + 17 * n + 3 * D + Z)
        self.dev, self.n, self.D, self.Z, self.dtype, self.n_slots = dev, n, D, Z, dtype, n_slots
        self.outs = tuple(o for o in outs if Z > 0 or o not in ('zc', 'zs', 'z_out'))
        pad4 = lambda w: (w + 3) // 4 * 4
        L = lambda key, default: lay.get(key, default)
        mean, std = stats(g, D)
        so = L('stat_off', 0)
        self.mean = Buf(dev, (D,), (1,), so, F32).put(mean)
        self.std = Buf(dev, (D,), (1,), so, F32).put(std)
        self.obs = Buf(dev, (n, D), (L('obs_ld', pad4(D) + 4), 1), L('obs_off', 4), F32).put(_steer(g, n, D, Y_SPECIAL, mean, std))
        self.z = None
        if Z > 0:
            self.z = Buf(dev, (n, Z), (L('z_ld', pad4(Z) + 8), 1), L('z_off', 8), F32).put(_steer(g, n, Z, Z_SPECIAL))
        self.bufs = {}
        for k, W in (('xa', D), ('xc', D), ('zc', Z), ('zs', Z)):
            if k in self.outs:
                wide = pad4(W) + 8                                   # the window is wider than W: columns at and beyond W stay
                self.bufs[k] = Buf(dev, (n, wide), (L(k + '_ld', wide + 4), 1), L(k + '_off', 4), dtype)
        for k, W in (('obses_out', D), ('z_out', Z)):
            if k in self.outs:
                ld = L(k + '_ld', pad4(W) + 4)
                self.bufs[k] = Buf(dev, (n_slots, n, W), (n * ld + L(k + '_ss_extra', 8), ld, 1), L(k + '_off', 4), F32)
        self.x_ref, self.z_ref = reference(self.obs.want_view, None if self.z is None else self.z.want_view, mean, std, dtype, dev)

    def kwargs(self, slot=0, slot_dev=None):
        kw = dict(z=None if self.z is None else self.z.view, slot=slot, slot_dev=slot_dev)
        if 'xa' in self.outs or 'xc' in self.outs:
            kw.update(mean=self.mean.view, std=self.std.view)
        kw.update({k: b.view for k, b in self.bufs.items()})
        return kw

    def vec(self):
        """(observation side, latent side) of the path condition on the tensors about to be launched."""
        b = self.bufs
        norm = 'xa' in b or 'xc' in b
        vo = vec_condition(self.obs.view, self.mean.view if norm else None, self.std.view if norm else None,
                           [b[k].view for k in ('xa', 'xc') if k in b], b['obses_out'].view if 'obses_out' in b else None)
        vz = self.Z > 0 and vec_condition(self.z.view, None, None, [b[k].view for k in ('zc', 'zs') if k in b],
                                          b['z_out'].view if 'z_out' in b else None)
        return vo, vz

    def expect(self, slot):
        """Write the reference into the twins; slot None: the call writes nothing."""
        if slot is None:
            return
        for k, b in self.bufs.items():
            if k in ('xa', 'xc'):
                b.want_view[:, :self.D] = self.x_ref
            elif k in ('zc', 'zs'):
                b.want_view[:, :self.Z] = self.z_ref
            else:
                src = self.obs.want_view if k == 'obses_out' else self.z.want_view
                b.want_view[slot].view(I32).copy_(src.view(I32))

    def run(self, be, slot=0, slot_dev=None, word=None, call=None, what=''):
        """Launch, then compare every allocation - inputs included - with its twin.  word: the value of the slot word."""
        vo, vz = self.vec()
        COUNTS['vec_obs_on' if vo else 'vec_obs_off'] += 1
        if self.Z:
            COUNTS['vec_z_on' if vz else 'vec_z_off'] += 1
        (call or be.rollout_head)(self.obs.view, **self.kwargs(slot, slot_dev))
        COUNTS['launches'] += 1
        slotted = 'obses_out' in self.bufs or 'z_out' in self.bufs
        s = slot if (word is None or not slotted) else (word if 0 <= word < self.n_slots else None)
        self.expect(s)
        self.check(what)

    def check(self, what=''):
        tag = (what, self.n, self.D, self.Z, str(self.dtype), self.outs)
        for k, b in self.bufs.items():
            b.check(tag + (k,))
        for k, b in (('obs', self.obs), ('z', self.z), ('mean', self.mean), ('std', self.std)):
            if b is not None:
                b.check(tag + (k, 'input'))


# ---- the checks both files run -----------------------------------------------------------------------------------------------
def check_shapes(be, dev, n, dtype):
    """Every D and Z at one row count and dtype, all outputs together; D 4 / 260 and Z 64 in the aligned layout take the 16-byte
    path, the others the 4-byte path."""
    for D in DS:
        for Z in ZS:
            c = Case(dev, n, D, Z, dtype)
            vo, vz = c.vec()
            assert vo == (D % 4 == 0) and vz == (Z == 64), (D, Z, vo, vz)
            c.run(be, slot=1, what='shapes')


# one clause of the path condition violated per entry: (layout knob, value, side that leaves the 16-byte path)
VIOLATIONS = (('obs_ld', 261, 'obs'), ('obs_off', 5, 'obs'), ('stat_off', 1, 'obs'), ('xa_ld', 277, 'obs'), ('xa_off', 5, 'obs'),
              ('xc_ld', 274, 'obs'), ('xc_off', 6, 'obs'), ('obses_out_ld', 263, 'obs'), ('obses_out_ss_extra', 6, 'obs'),
              ('obses_out_off', 3, 'obs'), ('z_ld', 65, 'z'), ('z_off', 7, 'z'), ('zc_ld', 77, 'z'), ('zc_off', 2, 'z'),
              ('zs_ld', 78, 'z'), ('zs_off', 1, 'z'), ('z_out_ld', 67, 'z'), ('z_out_ss_extra', 2, 'z'), ('z_out_off', 1, 'z'))


def check_violation(be, dev, dtype, knob, value, side):
    """n 65, D 260, Z 64 - on the 16-byte path on both sides (check_shapes asserts it) - with one clause violated: that side
    leaves the path, the other stays on it.  (D 253 / Z 1, off by the width alone, are check_shapes' cases.)"""
    c = Case(dev, 65, 260, 64, dtype, **{knob: value})
    assert c.vec() == (side != 'obs', side != 'z'), (knob, value, c.vec())
    c.run(be, slot=2, what=f'violated {knob}')


def check_one_row(be, dev, dtype):
    """n = 1: the row stride of a [1, W] view means nothing (0 or 1 after a select or an expand) and must not be taken for a
    pitch below the width."""
    for D, Z in ((260, 64), (253, 1)):
        Case(dev, 1, D, Z, dtype, obs_ld=1, z_ld=0, xa_ld=1, xc_ld=0, zc_ld=0, zs_ld=1, seed=13).run(be, slot=1, what='one row')


OUTPUT_SETS = tuple((o,) for o in OUTS) + (OUTS, CRITIC_ONLY, ('xa', 'zs'), ('obses_out', 'z_out'))


def check_outputs(be, dev, dtype, outs):
    for D, Z in ((253, 64), (260, 1), (4, 64)):
        Case(dev, 65, D, Z, dtype, outs=outs, seed=3).run(be, slot=0, what=f'outputs {outs}')


def check_slots(be, dev, dtype):
    """Slot 0 and n_slots - 1 by value and by word; a word at -1 and at n_slots: nothing at all is written."""
    word = torch.zeros(3, dtype=I32, device=dev)
    for v in (0, 3):
        Case(dev, 64, 260, 64, dtype, n_slots=4, seed=v).run(be, slot=v, what=f'slot {v} by value')
        word.copy_(torch.tensor([77, v, 78], dtype=I32))
        Case(dev, 64, 253, 1, dtype, n_slots=4, seed=v).run(be, slot=1, slot_dev=word[1:2], word=v, what=f'slot {v} by word')
    for v in (-1, 4):
        word.copy_(torch.tensor([77, v, 78], dtype=I32))
        for D in (253, 260):
            Case(dev, 65, D, 64, dtype, n_slots=4).run(be, slot=0, slot_dev=word[1:2], word=v, what=f'word {v}')
    # without a slot output the slot arguments are ignored: the word does not gate the normalised outputs
    Case(dev, 65, 260, 64, dtype, outs=('xa', 'xc', 'zc', 'zs')).run(be, slot=9, slot_dev=word[1:2], what='ignored slot arguments')
    assert word.cpu().tolist() == [77, 4, 78]


WORD_STEPS = [(start, add, wrap) for start in (0, 3, 2 ** 31 - 1, 2 ** 31 - 2, -2 ** 31, -1) for add in (1, 3) for wrap in (0, 4)]


def word_step_ref(start, add, wrap):
    v = start + add
    if wrap > 0:
        v %= wrap
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def check_word_step(be, dev, call=None):
    words = torch.zeros(3, dtype=I32, device=dev)
    for start, add, wrap in WORD_STEPS:
        words.copy_(torch.tensor([0x5A5A5A5A, start, 0x5A5A5A5A], dtype=torch.int64).to(I32))
        (call or be.word_step)(words[1:2], add, wrap)
        assert words.cpu().tolist() == [0x5A5A5A5A, word_step_ref(start, add, wrap), 0x5A5A5A5A], (start, add, wrap)
    # a counter: 0, 1, 2, 3, 0 under wrap 4
    seen = []
    words.zero_()
    for _ in range(5):
        seen.append(int(words[1]))
        (call or be.word_step)(words[1:2], 1, 4)
    assert seen == [0, 1, 2, 3, 0]


def check_program(be, dev, dtype):
    """A program with the head, rollout_store and word_step, recorded once - recording executes nothing - and replayed 4 times
    over 4 slots with the inputs rewritten in between, against four eager calls by value on a twin."""
    n, D, Z, S = 65, 253, 64, 4
    mk = lambda: Case(dev, n, D, Z, dtype, n_slots=S, seed=5)
    c, twin = mk(), mk()
    dones = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    dones_out = [torch.full((S, n), 9, dtype=torch.uint8, device=dev) for _ in range(2)]
    extra = [torch.zeros(n, 5, device=dev) for _ in range(2)]
    extra_out = [torch.full((S, n, 5), -7.0, device=dev) for _ in range(2)]
    word = torch.zeros(1, dtype=I32, device=dev)
    prog = be.prog_create()
    be.prog_begin(prog)
    try:
        be.rollout_head(c.obs.view, **c.kwargs(0, word))
        be.rollout_store(dones[0], slot=0, fields=[(extra[0], extra_out[0])], dones_out=dones_out[0], slot_dev=word)
        be.word_step(word, 1, 0)
    finally:
        be.prog_end(prog)
    assert be.prog_size(prog) == 3
    c.check('recording executes nothing')
    assert int(word) == 0 and bool((dones_out[0] == 9).all())
    g = torch.Generator().manual_seed(11)
    for s in range(S):
        obs = _steer(g, n, D, Y_SPECIAL, c.mean.want_view, c.std.want_view)
        zz = _steer(g, n, Z, Z_SPECIAL)
        d = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
        e = torch.randn(n, 5, generator=g)
        for k, cc in enumerate((c, twin)):
            cc.obs.put(obs)
            cc.z.put(zz)
            cc.x_ref, cc.z_ref = reference(obs, zz, cc.mean.want_view, cc.std.want_view, dtype, dev)
            dones[k].copy_(d)
            extra[k].copy_(e)
        be.prog_launch(prog)
        assert int(word) == s + 1
        c.expect(s)
        c.check(f'replay {s}')
        twin.run(be, slot=s, what=f'eager twin {s}')
        be.rollout_store(dones[1], slot=s, fields=[(extra[1], extra_out[1])], dones_out=dones_out[1])
        assert torch.equal(dones_out[0], dones_out[1]) and torch.equal(bits(extra_out[0]), bits(extra_out[1]))
        assert torch.equal(dones_out[0][s].cpu(), d)
    be.prog_launch(prog)                                   # the word is now 4 = n_slots: the fifth replay writes nothing
    c.check('a replay past the last slot')
    assert int(word) == S + 1
    be.prog_destroy(prog)
