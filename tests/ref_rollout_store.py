"""The reference of ``rollout_store`` - NOT the emulator - and the cases both test files run.

Three statements of what one environment step leaves behind:

  ``ref_step``        the lines of learning/common_agent.py:267-293 of the reference in torch, in the dtype handed in (f32: the
                      reference's own arithmetic, f64: the yardstick).  The boolean-index / ``nonzero`` form stays as the
                      reference writes it.
  ``meter_update``    rl_games ``AverageMeter.update`` restated in f64 python floats (the order of the sum: left to right).
  ``anchor_meters``   ``ase_amd.learning.agents.AverageMeter`` itself driven over the same values: the f32 anchor.

``WRONG`` names six single-term wrong restatements; ``ref_step`` / ``meter_update`` take one by name, so that a test can show
each one missing a bound.  ``run_case`` / ``run_meter_sequence`` build guarded allocations on a device, call a backend's
``rollout_store`` and check it against the statements above; tests/test_gpu_rollout_store.py runs them on the HIP backend,
tests/test_rollout_store_emu.py on the stand-in.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
import torch

from ase_amd.learning import agents

F32, F64 = torch.float32, torch.float64
NAN, INF = float('nan'), float('inf')
KINDS = (torch.uint8, torch.int32, torch.int64, torch.float32)
WRONG = ('shaped_into_accumulator', 'zeroed_before_meter', 'size_unclipped', 'old_uncut', 'terminate_from_dones',
         'length_not_incremented_on_done')
MAX_SIZE = 100
SEQ_DONE_COUNTS = (0, 5, 130, 30, 0, 80)        # per call of a meter sequence: k == 0, 0 < k < max, k >= max, a cut `old`
COUNTS = {'cases': 0, 'elements': 0, 'unequal': 0, 'guard_words': 0, 'meter_calls': 0}
STATS = {'meter |hip - f64| / allowance': 0.0, 'meter |hip - f64|': 0.0, 'meter |hip - f32 meter|': 0.0, 'meter e_ref': 0.0}


# ---- the reference's lines -----------------------------------------------------------------------------------------------------
def ref_step(rewards, dones, terminate, next_values, cur_rewards, cur_lengths, shift, scale, dtype=F32, wrong=None):
    """learning/common_agent.py:267-293 on one step's environment outputs.  rewards [N, 1], dones [N], terminate [N],
    next_values [N, 1], cur_rewards [N, 1], cur_lengths [N] -> dict of what the step stores, the values pushed into the two
    meters (in row order) and the accumulators behind the step.  Arithmetic in `dtype`."""
    rewards, next_values = rewards.to(dtype), next_values.to(dtype)
    cur_rewards, cur_lengths = cur_rewards.to(dtype).clone(), cur_lengths.to(dtype).clone()
    shaped_rewards = (rewards + shift) * scale
    flags = dones if wrong == 'terminate_from_dones' else terminate
    terminated = flags.to(dtype)
    terminated = terminated.unsqueeze(-1)
    next_vals = next_values.clone()
    next_vals *= (1.0 - terminated)
    cur_rewards += shaped_rewards if wrong == 'shaped_into_accumulator' else rewards
    if wrong == 'length_not_incremented_on_done':
        cur_lengths += (dones == 0).to(dtype)
    else:
        cur_lengths += 1
    all_done_indices = dones.nonzero(as_tuple=False)
    done_indices = all_done_indices[::1]
    not_dones = 1.0 - dones.to(dtype)
    if wrong == 'zeroed_before_meter':
        cur_rewards = cur_rewards * not_dones.unsqueeze(1)
        cur_lengths = cur_lengths * not_dones
    pushed_r, pushed_l = cur_rewards[done_indices], cur_lengths[done_indices]
    if wrong != 'zeroed_before_meter':
        cur_rewards = cur_rewards * not_dones.unsqueeze(1)
        cur_lengths = cur_lengths * not_dones
    done_indices = done_indices[:, 0]
    ids = torch.full((dones.numel(),), -1, dtype=torch.int32)
    ids[done_indices] = done_indices.to(torch.int32)
    return {'rewards_out': shaped_rewards, 'dones_out': (dones != 0).to(torch.uint8), 'next_values_out': next_vals,
            'cur_rewards': cur_rewards, 'cur_lengths': cur_lengths, 'pushed_r': pushed_r.reshape(-1), 'pushed_l': pushed_l.reshape(-1),
            'done_ids': ids}


def meter_update(mean, current_size, values, max_size, wrong=None):
    """AverageMeter.update (rl_games torch_ext) in f64: (mean, current_size) -> (mean, current_size)."""
    size = len(values)
    if size == 0:
        return mean, current_size
    total = 0.0
    for v in values:
        total += float(v)
    new_mean = total / size
    if wrong != 'size_unclipped':
        size = int(np.clip(size, 0, max_size))
    old_size = current_size if wrong == 'old_uncut' else min(max_size - size, current_size)
    size_sum = old_size + size
    return (mean * old_size + new_mean * size) / size_sum, size_sum


def meter_words(words, pushed_r, pushed_l, max_size, wrong=None):
    """The four device words {reward mean, length mean, current size, episodes seen} behind one call."""
    mr, size = meter_update(words[0], words[2], pushed_r.double().tolist(), max_size, wrong)
    ml, _ = meter_update(words[1], words[2], pushed_l.double().tolist(), max_size, wrong)
    return [mr, ml, float(size), words[3] + len(pushed_r)]


def meter_allowance(prev_mean, values):
    """|hip - f64| <= (k + 8) 2^-53 max(|previous mean|, max |x|): k - 1 additions of the sum in any order, the division, two
    products, a sum and a division of the update, each within half an ulp of a quantity no larger than that maximum."""
    k = len(values)
    return (k + 8) * 2.0 ** -53 * max(abs(prev_mean), max((abs(float(v)) for v in values), default=0.0))


def anchor_meters(max_size, start_size=0, start_means=(0.0, 0.0)):
    """The two host meters of the agents as they stand, optionally started from a state."""
    mr, ml = agents.AverageMeter(1, max_size), agents.AverageMeter(1, max_size)
    for m, v in ((mr, start_means[0]), (ml, start_means[1])):
        m.current_size = start_size
        m.mean.fill_(v)
    return mr, ml


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def done_pattern(name, n, gen, count=None):
    d = torch.zeros(n, dtype=torch.bool)
    if name == 'all':
        d[:] = True
    elif name == 'row0':
        d[0] = True
    elif name == 'last':
        d[n - 1] = True
    elif name == 'random':
        d = torch.rand(n, generator=gen) < 0.125
    elif name == 'count':
        d[torch.randperm(n, generator=gen)[:count]] = True
    else:
        assert name == 'none'
    return d


def vec_path(src, dst):
    """rollout_store_kernel's condition for 16 bytes per lane (csrc/rollout_store.hip), on a (source [N, D], destination
    [S, N, D]) pair of views."""
    D = src.shape[1]
    return (D % 4 == 0 and src.stride(0) % 4 == 0 and dst.stride(1) % 4 == 0 and dst.stride(0) % 4 == 0 and
            src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == F32 else (t.view(torch.int64) if t.dtype == F64 else t)


def same(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = int((g != w).sum())
    COUNTS['elements'] += g.numel()
    COUNTS['unequal'] += bad
    assert bad == 0, f'{what}: {bad} of {g.numel()} elements differ bitwise'


class Guarded:
    """A window of a sentinel-filled allocation: `win` is handed to the launch, check() proves that nothing outside the
    elements `written` (a boolean mask over the allocation, None: nothing) changed."""

    def __init__(self, alloc, win):
        self.alloc, self.win, self.before = alloc, win, alloc.clone()

    def check(self, written, what):
        a, b = bits(self.alloc), bits(self.before)
        changed = a != b
        if written is not None:
            changed = changed & ~written.cpu().reshape(changed.shape)
            COUNTS['guard_words'] += int((~written).sum())
        else:
            COUNTS['guard_words'] += a.numel()
        assert not bool(changed.any()), f'{what}: {int(changed.sum())} words outside the window were written'
        self.before = self.alloc.clone()


def sentinel(shape, dtype, dev):
    if dtype in (F32, F64):
        return torch.full(shape, NAN, dtype=dtype, device=dev)
    return torch.full(shape, 0xAB if dtype == torch.uint8 else -7, dtype=dtype, device=dev)


class Step:
    """One call's operands inside guarded allocations.  fields: [(D, extra pitch, misalign)]: the source is [N, D + extra], the
    destination [S, N + 1, D + extra] of which [S, N, D] is the window.  misalign: True / 'src' - the source starts one float
    off 16-byte alignment; 'dst' - the destination does; 'ss' - the slot stride is one float longer (odd for D % 4 == 0)."""

    def __init__(self, dev, n, n_slots=3, fields=(), dones_dtype=torch.uint8, term_dtype=torch.bool, seed=0):
        g = self.gen = torch.Generator().manual_seed(seed)
        self.dev, self.n, self.S = dev, n, n_slots
        self.src, self.dst = [], []
        for D, extra, misalign in fields:
            ld = D + extra
            raw = sentinel((n * ld + 8,), F32, dev)
            off = 1 if misalign in (True, 'src') else 0
            s = raw[off:off + n * ld].view(n, ld)[:, :D]
            s.copy_(torch.randn(n, D, generator=g))
            ss = (n + 1) * ld + (1 if misalign == 'ss' else 0)
            flat = sentinel((n_slots * ss + 8,), F32, dev)
            win = flat.as_strided((n_slots, n, D), (ss, ld, 1), 1 if misalign == 'dst' else 0)
            self.src.append(s)
            self.dst.append(Guarded(flat, win))
        self.dones_dtype, self.term_dtype = dones_dtype, term_dtype
        # the launch's inputs live at fixed device addresses (a recorded launch reads them again): inputs() rewrites them
        self.d_rewards, self.d_next_values = torch.zeros(n, 1, device=dev), torch.zeros(n, 1, device=dev)
        self.d_dones = torch.zeros(n, dtype=dones_dtype, device=dev)
        self.d_terminate = torch.zeros(n, dtype=term_dtype, device=dev)
        self.rewards_out = self._slotted(F32)
        self.dones_out = self._slotted(torch.uint8)
        self.next_values_out = self._slotted(F32)
        ids = sentinel((n + 2,), torch.int32, dev)
        self.done_ids = Guarded(ids, ids[1:n + 1])
        cr, cl = sentinel((n + 2,), F32, dev), sentinel((n + 2,), F32, dev)
        self.cur_rewards, self.cur_lengths = Guarded(cr, cr[1:n + 1]), Guarded(cl, cl[1:n + 1])
        self.cur_rewards.win.copy_(torch.rand(n, generator=g) * 50.0)
        self.cur_lengths.win.copy_(torch.randint(0, 300, (n,), generator=g).float())
        m = sentinel((6,), F64, dev)
        self.meter = Guarded(m, m[1:5])
        self.meter.win.zero_()
        self.inputs(done_pattern('random', n, g))
        for gd in self.guarded():
            gd.before = gd.alloc.clone()

    def _slotted(self, dtype):
        big = sentinel((self.S, self.n + 3), dtype, self.dev)
        return Guarded(big, big[:, :self.n])

    def inputs(self, dones, terminate=None, rewards=None):
        g, n = self.gen, self.n
        self.rewards = (torch.rand(n, 1, generator=g) * 2.0) if rewards is None else rewards.view(n, 1).clone()
        self.next_values = torch.randn(n, 1, generator=g)
        self.dones = dones.to(self.dones_dtype)
        t = (dones & (torch.rand(n, generator=g) < 0.5)) if terminate is None else terminate
        self.terminate = t.to(self.term_dtype)
        for x in self.src:
            x.copy_(torch.randn(x.shape, generator=g))
        for d, h in ((self.d_rewards, self.rewards), (self.d_next_values, self.next_values), (self.d_dones, self.dones),
                     (self.d_terminate, self.terminate)):
            d.copy_(h)

    def start_meter(self, mean_r, mean_l, size, seen=0.0):
        self.meter.win.copy_(torch.tensor([mean_r, mean_l, float(size), seen], dtype=F64))
        self.meter.before = self.meter.alloc.clone()

    def kwargs(self, slot, shift, scale, leave_out=(), slot_dev=None):
        dev = self.dev
        kw = dict(slot=slot, n_slots=self.S, fields=[(s, d.win) for s, d in zip(self.src, self.dst)], shift=shift, scale=scale,
                  slot_dev=slot_dev)
        if 'rewards' not in leave_out or 'accumulators' not in leave_out:
            kw['rewards'] = self.d_rewards
        if 'rewards' not in leave_out:
            kw['rewards_out'] = self.rewards_out.win
        if 'dones_out' not in leave_out:
            kw['dones_out'] = self.dones_out.win
        if 'next_values' not in leave_out:
            kw.update(next_values=self.d_next_values, terminate=self.d_terminate, next_values_out=self.next_values_out.win)
        if 'accumulators' not in leave_out:
            kw.update(cur_rewards=self.cur_rewards.win, cur_lengths=self.cur_lengths.win, meter=self.meter.win, max_size=MAX_SIZE)
        if 'done_ids_out' not in leave_out:
            kw['done_ids_out'] = self.done_ids.win
        return kw

    def expect(self, shift, scale, dtype=F32, wrong=None):
        return ref_step(self.rewards, self.dones, self.terminate, self.next_values, self.cur_rewards.win.cpu().view(-1, 1),
                        self.cur_lengths.win.cpu(), shift, scale, dtype, wrong)

    def run(self, be, slot, shift=0.0, scale=1.0, leave_out=(), slot_dev=None, word=None, what='', call=None, wrong=None):
        """One call checked against the f32 run of the reference, bitwise, every guard word included.  word: the value of the
        device slot word (None: the slot argument counts).  -> (reference dict, meter words before, meter words after)."""
        ref = self.expect(shift, scale, wrong=wrong)
        words0 = self.meter.win.cpu().tolist()
        kw = self.kwargs(slot, shift, scale, leave_out, slot_dev)
        (call or be.rollout_store)(self.d_dones, **kw)
        if self.dev != 'cpu':
            torch.cuda.synchronize()
        return self.check(ref, words0, slot if word is None else word, leave_out, what)

    def guarded(self):
        return self.dst + [self.rewards_out, self.dones_out, self.next_values_out, self.done_ids, self.cur_rewards,
                           self.cur_lengths, self.meter]

    def untouched(self, what):
        for g in self.guarded():
            g.check(None, what)

    def check(self, ref, words0, slot, leave_out=(), what=''):
        n, S = self.n, self.S
        live = 0 <= slot < S                                       # a slot word outside the buffer: nothing anywhere
        for s, d in zip(self.src, self.dst):
            mask = torch.zeros(d.alloc.shape, dtype=torch.bool)
            if live:                                               # the window's elements of this slot, wherever they lie
                mask.as_strided(d.win.shape, d.win.stride(), d.win.storage_offset() - d.alloc.storage_offset())[slot] = True
                same(d.win[slot], s, f'{what} field D{s.shape[1]}')
            d.check(mask if live else None, f'{what} field D{s.shape[1]}')
        for name, g, key in (('rewards', self.rewards_out, 'rewards_out'), ('dones_out', self.dones_out, 'dones_out'),
                             ('next_values', self.next_values_out, 'next_values_out')):
            on = live and name not in leave_out
            mask = torch.zeros(g.alloc.shape, dtype=torch.bool)
            if on:
                mask[slot, :n] = True
                same(g.win[slot], ref[key].reshape(-1), f'{what} {key}')
            g.check(mask if on else None, f'{what} {key}')
        on = live and 'done_ids_out' not in leave_out
        if on:
            same(self.done_ids.win, ref['done_ids'], f'{what} done_ids')
        self.done_ids.check(self._inner(n) if on else None, f'{what} done_ids')
        on = live and 'accumulators' not in leave_out
        if on:
            same(self.cur_rewards.win, ref['cur_rewards'].reshape(-1), f'{what} cur_rewards')
            same(self.cur_lengths.win, ref['cur_lengths'], f'{what} cur_lengths')
        self.cur_rewards.check(self._inner(n) if on else None, f'{what} cur_rewards')
        self.cur_lengths.check(self._inner(n) if on else None, f'{what} cur_lengths')
        words = self.meter.win.cpu().tolist()
        k = ref['pushed_r'].numel()
        if on and k > 0:
            inner = torch.zeros(6, dtype=torch.bool)
            inner[1:5] = True
            self.meter.check(inner, f'{what} meter')
        else:
            self.meter.check(None, f'{what} meter')                # k == 0 or no meter: bitwise unchanged, every word
        COUNTS['cases'] += 1
        return ref, words0, words

    @staticmethod
    def _inner(n):
        m = torch.zeros(n + 2, dtype=torch.bool)
        m[1:n + 1] = True
        return m


def check_meter(words0, words, ref, wrong=None):
    """One call's meter against the f64 restatement started from the words the call found (finite values only)."""
    want = meter_words(words0, ref['pushed_r'], ref['pushed_l'], MAX_SIZE, wrong)
    assert words[2] == want[2] and words[3] == want[3], ('current_size / episodes_seen', words, want)
    for i, key in ((0, 'pushed_r'), (1, 'pushed_l')):
        allow = meter_allowance(words0[i], ref[key].tolist())
        err = abs(words[i] - want[i])
        STATS['meter |hip - f64|'] = max(STATS['meter |hip - f64|'], err)
        if allow > 0:
            STATS['meter |hip - f64| / allowance'] = max(STATS['meter |hip - f64| / allowance'], err / allow)
        assert err <= allow, (key, err, allow)
    COUNTS['meter_calls'] += 1
    return want


def run_meter_sequence(be, dev, n, start_size, seed=11, call=None):
    """Six calls whose done counts meet the fixture conditions, from an empty meter or from current_size = 60: per call and
    accumulated against the f64 restatement, and against agents.AverageMeter in f32.  -> the words after every call."""
    st = Step(dev, n, n_slots=2, fields=[(5, 0, False)], seed=seed)
    start = (12.5, 140.25) if start_size else (0.0, 0.0)
    st.start_meter(start[0], start[1], start_size)
    mr, ml = anchor_meters(MAX_SIZE, start_size, start)
    chain, budget, seen, history = [start[0], start[1], float(start_size), 0.0], [0.0, 0.0], set(), []
    for i, k in enumerate(SEQ_DONE_COUNTS):
        st.inputs(done_pattern('count', n, st.gen, k))
        ref, words0, words = st.run(be, i % 2, shift=-0.5, scale=0.01, what=f'meter sequence call {i}', call=call)
        assert ref['pushed_r'].numel() == k
        if k == 0:
            assert bits(torch.tensor(words[:3], dtype=F64)).tolist() == bits(torch.tensor(words0[:3], dtype=F64)).tolist()
            seen.add('k == 0')
        else:
            size = min(k, MAX_SIZE)
            seen.add('0 < k < max_size' if k < MAX_SIZE else 'k >= max_size')
            if MAX_SIZE - size < words0[2]:
                seen.add('old cut')
        check_meter(words0, words, ref)
        # accumulated: the chain from the start in f64; a call's deviation enters the next mean with a weight old / (old +
        # size) <= 1, so the sum of the per-call allowances bounds it
        for j, key in ((0, 'pushed_r'), (1, 'pushed_l')):
            budget[j] += meter_allowance(chain[j], ref[key].tolist())
        chain = meter_words(chain, ref['pushed_r'], ref['pushed_l'], MAX_SIZE)
        mr.update(ref['pushed_r'].view(-1, 1))
        ml.update(ref['pushed_l'].view(-1, 1))
        assert words[2] == chain[2] == mr.current_size and words[3] == chain[3]
        for j, anchor in ((0, mr), (1, ml)):
            assert abs(words[j] - chain[j]) <= budget[j], (i, j, words[j], chain[j], budget[j])
            a = float(anchor.mean.double())
            e_ref = abs(a - chain[j])
            STATS['meter e_ref'] = max(STATS['meter e_ref'], e_ref)
            STATS['meter |hip - f32 meter|'] = max(STATS['meter |hip - f32 meter|'], abs(words[j] - a))
            assert abs(words[j] - a) <= 2.0 * e_ref + 2.0 ** -23 * abs(chain[j]), (i, j, words[j], a, e_ref)
        history.append(words)
    assert seen == {'k == 0', '0 < k < max_size', 'k >= max_size', 'old cut'}, seen
    return history


# ---- the cases -----------------------------------------------------------------------------------------------------------------
N_ENVS = (1, 63, 64, 65, 257, 1030)
WIDTHS = (1, 3, 31, 64, 253, 1400)
PATTERNS = ('none', 'all', 'row0', 'last', 'random')
SHAPERS = ((0.0, 1.0), (-0.5, 0.01))


def width_fields():
    """Every width with ld = D and ld = D + 7, and a width-64 field with the source, the destination or the slot stride one
    float off - each remaining term of the kernel's condition decides once -> (fields, expected 16-byte path)."""
    fields = [(D, extra, False) for D in WIDTHS for extra in (0, 7)] + [(64, 0, 'src'), (64, 0, 'dst'), (64, 0, 'ss')]
    paths = [D % 4 == 0 and extra == 0 for D in WIDTHS for extra in (0, 7)] + [False, False, False]
    return fields, paths


def special_rewards(n, dones, gen, done_vals=(NAN, INF)):
    """Non-finite rewards in done rows (done_vals) and a NaN and a -inf in live rows (where the pattern has both)."""
    r = torch.rand(n, generator=gen) * 2.0
    for rows, vals in ((dones.nonzero().flatten().tolist(), done_vals), ((~dones).nonzero().flatten().tolist(), (NAN, -INF))):
        for e, v in zip(rows[:2], vals):
            r[e] = v
    return r


def _finite_meter(st, ref, w0, w, leave_out=()):
    if 'accumulators' not in leave_out and bool(torch.isfinite(ref['pushed_r']).all()):
        check_meter(w0, w, ref)


def check_widths(be, dev):
    """Every width at both pitches and the three misaligned fields in ONE call of 15 fields, slots 0 and n_slots - 1; which path each
    field takes is what the kernel's condition says of these allocations."""
    fields, paths = width_fields()
    st = Step(dev, 65, n_slots=3, fields=fields, seed=2)
    assert [vec_path(s, d.win) for s, d in zip(st.src, st.dst)] == paths
    for slot, (shift, scale) in zip((0, 2), SHAPERS):
        st.inputs(done_pattern('random', st.n, st.gen))
        _finite_meter(st, *st.run(be, slot, shift, scale, what=f'widths slot {slot}'))


def check_n_envs(be, dev, n):
    """Every done pattern at one size, both shapers, first and last slot."""
    st = Step(dev, n, n_slots=2, fields=[(31, 0, False), (64, 0, False), (253, 7, False)], seed=100 + n)
    for i, pat in enumerate(PATTERNS):
        st.inputs(done_pattern(pat, n, st.gen))
        shift, scale = SHAPERS[i % 2]
        _finite_meter(st, *st.run(be, i % 2, shift, scale, what=f'n_envs {n} {pat}'))


def check_n_fields(be, dev, n_fields):
    st = Step(dev, 65, n_slots=2, fields=[(1 + 3 * i, i % 3, False) for i in range(n_fields)], seed=7 + n_fields)
    _finite_meter(st, *st.run(be, 1, -0.5, 0.01, what=f'{n_fields} fields'))


def check_kinds(be, dev, dones_dtype, term_dtype):
    st = Step(dev, 65, n_slots=2, fields=[(3, 0, False)], dones_dtype=dones_dtype, term_dtype=term_dtype, seed=31)
    for i, pat in enumerate(('random', 'all', 'none')):
        st.inputs(done_pattern(pat, st.n, st.gen))
        _finite_meter(st, *st.run(be, i % 2, -0.5, 0.01, what=f'kinds {dones_dtype} {term_dtype} {pat}'))


def check_special(be, dev):
    """NaN and +-inf rewards in done and live rows: every stored output is the f32 run of the reference, NaN pattern included,
    and the meter is what the f64 restatement holds - a NaN where it has one, a signed infinity by equality, a finite word
    within the allowance of its finite values; current_size and episodes_seen exactly.  Done rows with a NaN and a +inf give a
    NaN mean, with +inf alone +inf, with -inf alone -inf, with both infinities NaN."""
    seen = set()
    cases = [(pat, (NAN, INF)) for pat in ('random', 'all', 'none')] + [('random', (INF,)), ('random', (-INF,)), ('random', (INF, -INF))]
    for i, (pat, done_vals) in enumerate(cases):
        st = Step(dev, 65, n_slots=2, fields=[(3, 0, False)], seed=41)      # (fresh accumulators: a live row keeps its NaN)
        dones = done_pattern(pat, st.n, st.gen)
        st.inputs(dones, rewards=special_rewards(st.n, dones, st.gen, done_vals))
        st.start_meter(3.0, 40.0, 10, seen=7.0)
        ref, w0, w = st.run(be, i % 2, *SHAPERS[i % 2], what=f'special {pat} {done_vals}')
        want = meter_words(w0, ref['pushed_r'], ref['pushed_l'], MAX_SIZE)
        assert w[2] == want[2] and w[3] == want[3], ('current_size / episodes_seen', w, want)
        for j, key in ((0, 'pushed_r'), (1, 'pushed_l')):
            if math.isnan(want[j]):
                assert math.isnan(w[j]), (pat, done_vals, j, w, want)
            elif math.isinf(want[j]):
                assert w[j] == want[j], (pat, done_vals, j, w, want)
                seen.add(want[j])
            else:
                finite = [v for v in ref[key].tolist() if math.isfinite(v)]
                assert abs(w[j] - want[j]) <= meter_allowance(w0[j], finite), (pat, done_vals, j, w, want)
        seen.add('nan' if math.isnan(want[0]) else 'number')
        assert bool(torch.isnan(ref['rewards_out']).any()) and bool(torch.isinf(ref['rewards_out']).any())
    assert seen == {'nan', 'number', INF, -INF}, seen


GROUPS = ('rewards', 'dones_out', 'next_values', 'accumulators', 'done_ids_out')


def check_groups(be, dev):
    """Each nullable group left out in turn: its outputs keep every sentinel, the others are what they are with it."""
    for grp in GROUPS:
        st = Step(dev, 65, n_slots=2, fields=[(3, 0, False), (64, 0, False)], seed=51)
        _finite_meter(st, *st.run(be, 1, -0.5, 0.01, leave_out=(grp,), what=f'without {grp}'), leave_out=(grp,))
    st = Step(dev, 65, n_slots=2, fields=[], seed=52)
    st.run(be, 0, leave_out=GROUPS, what='dones alone')          # nothing to do: nothing written


def check_slot_word(be, dev):
    """Two slots followed through the device word; -1 and n_slots write nothing anywhere."""
    st = Step(dev, 65, n_slots=3, fields=[(3, 0, False), (64, 0, False)], seed=61)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    for v in (2, 1, -1, 3):
        word.fill_(v)
        st.inputs(done_pattern('random', st.n, st.gen))
        ref, w0, w = st.run(be, 0, -0.5, 0.01, slot_dev=word, word=v, what=f'slot word {v}')
        if 0 <= v < 3:
            check_meter(w0, w, ref)


def report():
    return {'counts': dict(COUNTS), 'stats': dict(STATS)}


assert math.isclose(meter_allowance(1.0, [1.0, 1.0]), 10 * 2.0 ** -53)
