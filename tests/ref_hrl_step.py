"""The reference of ``hrl_latent`` / ``hrl_llc_action`` / ``hrl_accum`` - NOT the emulator - and the cases both
test files run.

The reference's own lines in torch, in the dtype handed in (f32 on the CPU: the bitwise anchor, f64: the accuracy yardstick):

  ``ref_latent``      learning/hrl_agent.py:89-93,235      z = F.normalize(torch.clamp(actions, -1, 1), dim=-1)
  ``ref_llc_action``  learning/hrl_agent.py:238 through ASEAgent.preprocess_actions: rl_games rescale_actions(low, high,
                      torch.clamp(mu, -1, 1)); without clip_actions the head output itself
  ``ref_fold``        learning/hrl_agent.py:45-82           the four running sums over the inner steps (each starts from the float
                      0.0), the two means ``sum / llc_steps`` and the two ``(count > 0)`` masks

``WRONG`` names five single-term wrong restatements; the functions take one by name, so that a test can show each one missing a
bar.  ``check_latent`` / ``check_llc_action`` / ``check_accum`` build guarded allocations on a device, call a backend and check
it against the lines above; tests/test_gpu_hrl_step.py runs them on the HIP backend, tests/test_hrl_step_emu.py on the
stand-in.  TEST INFRASTRUCTURE ONLY.

The bars.  Bitwise wherever the arithmetic is a fixed sequence of correctly rounded f32 operations (the clamp, rescale_actions,
the sums, the division, the masks).  Where a transcendental or a sum order enters:
  z            bitwise the device's own ``normalize_rows(torch.clamp(a, -1, 1))`` (one row code), and against f64 at the bar
               tests/ref_rollout.py holds normalize_rows to, 2 e_ref + 1e-7 (``RR.within``).
  disc_out     the per-step rewards come from the device's own ``disc_reward`` and enter the f32 reference lines: bitwise.  Against
               f64: each step's reward may be off by a_t = 2 e_t + 1e-7 (the bar tests/test_gpu_rollout.py holds disc_reward to,
               e_t = max |f32 reference - f64| of that step); the f32 fold adds at most T roundings of 2^-24 max |sum| and the
               division one more of 2^-24 |mean|, and max |sum| = T max |mean|.  So
                   |disc_out - f64| <= mean_t(a_t) + (T + 1) 2^-24 max |mean_f64|.
  agents       ``rewards`` / ``disc_rewards`` of a key agent against the default path: bitwise at llc_steps 2 and 4 (x / T is exact
               scaling or rounds the same either way), within 2^-22 |ref| + 2^-149 at 3 and 5 - a torch build may compute
               x / T as x * RN(1 / T): two roundings of 2^-24 against the kernel's one."""
import sys

import torch
import torch.nn.functional as F

from ase_amd.learning.agents import rescale_actions
from tests import ref_rollout as RR

F32, F64 = torch.float32, torch.float64
NAN, INF = float('nan'), float('inf')
KINDS = (torch.uint8, torch.int32, torch.int64, torch.float32)
STORAGE = (torch.float32, torch.bfloat16, torch.float16)
WRONG = ('reciprocal_multiply', 'clamp_after_rescale', 'dones_last_step_only', 'count_ge_one', 'normalize_before_clamp')
DISC_SCALE = 2.0
COUNTS = {'calls': 0, 'elements': 0, 'unequal': 0, 'guard_words': 0}
STATS = {'z |got - f64|': 0.0, 'z e_ref': 0.0, 'disc_out |got - f64|': 0.0, 'disc_out allowance': 0.0,
         'agent rewards |key - default| / |default|': 0.0}

LATENT_N, LATENT_DIM = (1, 4, 5, 257), (1, 63, 64, 65, 128)
ACTION_N, ACTION_ACT, ACTION_PITCH = (1, 63, 64, 65, 1030), (1, 28, 31, 64, 128), (64, 128)
ACCUM_N, ACCUM_T = (1, 63, 64, 65, 257, 1030), (1, 2, 3, 5)
PLANTS = (1.0, -1.0, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 100.0, -100.0, INF, -INF, NAN, -0.0)


# ---- the reference's lines -----------------------------------------------------------------------------------------------------
def ref_latent(actions, dtype=F32, wrong=None):
    a = actions.to(dtype)
    if wrong == 'normalize_before_clamp':
        return torch.clamp(F.normalize(a, dim=-1), -1.0, 1.0)
    return F.normalize(torch.clamp(a, -1.0, 1.0), dim=-1)


def ref_llc_action(mu, low, high, clip=True, dtype=F32, wrong=None):
    mu, low, high = mu.to(dtype), low.to(dtype), high.to(dtype)
    if not clip:
        return mu
    if wrong == 'clamp_after_rescale':
        return torch.clamp(rescale_actions(low, high, mu), -1.0, 1.0)
    return rescale_actions(low, high, torch.clamp(mu, -1.0, 1.0))


def ref_fold(rewards, dones, terminate, disc, llc_steps, dtype=F32, wrong=None):
    """hrl_agent.py:57-73 over per-step lists (terminate / disc: a list or None).  Returns (partials, finals): partials[t] = the
    four running sums after inner step t (None for an absent group), finals = rewards, disc_rewards, dones, terminate."""
    r = dr = d = tc = 0.0
    partials = []
    for t in range(llc_steps):
        r = r + rewards[t].to(dtype)
        d = d + dones[t].to(dtype)
        if wrong == 'dones_last_step_only':
            d = dones[t].to(dtype)
        if disc is not None:
            dr = dr + disc[t].to(dtype)
        if terminate is not None:
            tc = tc + terminate[t].to(dtype)
        partials.append((r, dr if disc is not None else None, d, tc if terminate is not None else None))
    if wrong == 'reciprocal_multiply':
        inv = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(llc_steps), dtype=dtype)
        mean = lambda x: x * inv
    else:
        mean = lambda x: x / llc_steps
    mask = (lambda c: (c >= 1).to(dtype)) if wrong == 'count_ge_one' else (lambda c: (c > 0).to(dtype))
    finals = (mean(r), mean(dr) if disc is not None else None, mask(d), mask(tc) if terminate is not None else None)
    return partials, finals


def agent_reward_bar(got, ref, llc_steps, what):
    """rewards / disc_rewards of a key agent against the default path (module docstring)."""
    g, w = got.detach().cpu().reshape(-1), ref.detach().cpu().reshape(-1)
    if llc_steps in (1, 2, 4):
        same(g, w, what)
        return
    err = (g.double() - w.double()).abs()
    tol = 2.0 ** -22 * w.double().abs() + 2.0 ** -149
    rel = float((err / w.double().abs().clamp_min(1e-30)).max())
    STATS['agent rewards |key - default| / |default|'] = max(STATS['agent rewards |key - default| / |default|'], rel)
    print(f'{what}: max |key - default| / |default| = {rel:.3g} (bar 2^-22 = {2.0 ** -22:.3g})')
    assert bool((err <= tol).all()), (what, float(err.max()))


# ---- guarded allocations -------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == F32:
        return t.view(torch.int32)
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16)
    return t.view(torch.int64) if t.dtype == F64 else t


def same(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape and got.dtype == want.dtype, (what, g.shape, w.shape, got.dtype, want.dtype)
    bad = int((g != w).sum())
    COUNTS['elements'] += g.numel()
    COUNTS['unequal'] += bad
    assert bad == 0, f'{what}: {bad} of {g.numel()} elements differ bitwise'


class Guarded:
    """A window of a sentinel-filled allocation with a wider pitch: `win` is handed to the launch, check() proves that nothing
    outside the window changed since the last look (written=False: nothing at all)."""

    def __init__(self, shape, dtype, dev, pad=(1, 5), fill=NAN):
        full = tuple(s + p for s, p in zip(shape, pad))
        self.alloc = torch.full(full, fill, dtype=dtype, device=dev)
        self.win = self.alloc[tuple(slice(0, s) for s in shape)]
        self.mask = torch.zeros(full, dtype=torch.bool)
        self.mask[tuple(slice(0, s) for s in shape)] = True
        self.before = self.alloc.clone()

    def check(self, what, written=True):
        a, b = bits(self.alloc), bits(self.before)
        changed = a != b
        if written:
            changed = changed & ~self.mask
            COUNTS['guard_words'] += int((~self.mask).sum())
        else:
            COUNTS['guard_words'] += a.numel()
        assert not bool(changed.any()), f'{what}: {int(changed.sum())} words outside the window were written'
        self.before = self.alloc.clone()


def vec(n, dtype, dev, fill=NAN):
    """A guarded [n] vector: a window of a longer sentinel-filled allocation."""
    if dtype not in (F32, F64):
        fill = 0xAB if dtype == torch.uint8 else -7
    return Guarded((n,), dtype, dev, pad=(9,), fill=fill)


# ---- hrl_latent ----------------------------------------------------------------------------------------------------------------
def latent_actions(n, dim, gen):
    """High-level actions: N(0, 1.5^2) (a third of the elements beyond +-1), +-1 and -0.0 planted; from 4 rows on a zero row (the
    norm floor), a 1e-20 row (a norm below the floor, squares subnormal) and a row with a NaN."""
    a = torch.randn(n, dim, generator=gen) * 1.5
    flat = a.view(-1)
    for i, v in enumerate((1.0, -1.0, -0.0)[:flat.numel()]):
        flat[flat.numel() - 1 - i] = v
    special = {}
    if n >= 4:
        a[0] = 0.0
        a[1] = 1e-20
        a[2, dim // 2] = NAN
        special = {'zero': 0, 'tiny': 1, 'nan': 2}
    return a, special


def check_latent(be, dev, n, dim, extra, seed=5):
    """z bitwise the backend's own normalize_rows(torch.clamp(a, -1, 1)), z2 in the three storage types bitwise the gather_rows
    conversion of z, z within the normalize_rows bar of f64; the special rows as tensors of their own; pad columns intact."""
    gen = torch.Generator().manual_seed(seed + 131 * n + dim)
    a, special = latent_actions(n, dim, gen)
    src = torch.full((n, dim + extra), NAN)
    src[:, :dim] = a
    src = src.to(dev)
    want = torch.empty(n, dim, dtype=F32, device=dev)
    be.normalize_rows(torch.clamp(src[:, :dim], -1.0, 1.0).contiguous(), want, n, dim)
    z64, z32 = ref_latent(a, F64), ref_latent(a, F32)
    for dt in STORAGE + (None,):
        z = Guarded((n, dim), F32, dev)
        z2 = None if dt is None else Guarded((n, dim), dt, dev, pad=(1, 64 - dim % 64), fill=3.0)
        be.hrl_latent(src[:, :dim], z=z.win, z2=None if z2 is None else z2.win, dim=dim)
        COUNTS['calls'] += 1
        what = f'hrl_latent n {n} dim {dim} ld_a {dim + extra} z2 {dt}'
        z.check(what)
        same(z.win, want, what + ': z against normalize_rows(clamp)')
        if z2 is not None:
            z2.check(what + ' z2')
            conv = torch.zeros(n, dim, dtype=dt, device=dev)
            be.gather_rows(z.win.contiguous(), dim, None, (0, 0), n, conv)
            same(z2.win, conv, what + ': z2 against the gather_rows conversion of z')
            # z2 alone (z NULL): the same bits
            only = Guarded((n, dim), dt, dev, pad=(1, 64 - dim % 64), fill=3.0)
            be.hrl_latent(src[:, :dim], z2=only.win, dim=dim)
            only.check(what + ' z2 alone')
            same(only.win, z2.win, what + ': z2 without z')
    err, e_ref = RR.within(z.win, z64, z32, f'hrl_latent n {n} dim {dim}')
    STATS['z |got - f64|'], STATS['z e_ref'] = max(STATS['z |got - f64|'], err), max(STATS['z e_ref'], e_ref)
    got = z.win.cpu()
    for name, row in special.items():
        same(got[row], z32[row] if name != 'nan' else torch.full((dim,), NAN), f'{name} row')     # F.normalize: a NaN fills its row
    if special:
        assert bool((got[0] == 0).all()) and bool(torch.isnan(got[2]).all())
        assert torch.equal(got[1], torch.full((dim,), 1e-20) / torch.tensor(1e-12))
    return a, got


# ---- hrl_llc_action ------------------------------------------------------------------------------------------------------------
def action_case(n, act, gen):
    """The head output: N(0, 1.2^2) (about 40 % beyond +-1) with PLANTS at the front; asymmetric bounds, one joint with
    low == high."""
    mu = torch.randn(n, act, generator=gen) * 1.2
    flat = mu.view(-1)
    k = min(flat.numel(), len(PLANTS))
    flat[:k] = torch.tensor(PLANTS[:k])
    low = -(torch.rand(act, generator=gen) * 2.0 + 0.1)
    high = torch.rand(act, generator=gen) * 3.0 + 0.2
    if act > 1:
        high[act // 2] = low[act // 2]
    return mu, low, high


def check_llc_action(be, dev, n, act, pitch, seed=7):
    gen = torch.Generator().manual_seed(seed + 17 * n + act)
    mu, low, high = action_case(n, act, gen)
    head = torch.full((n, pitch), NAN)                    # the padded head output: columns past act are never read
    head[:, :act] = mu
    head, lo, hi = head.to(dev), low.to(dev), high.to(dev)
    for clip in (True, False):
        out = Guarded((n, act), F32, dev)
        be.hrl_llc_action(head, lo if clip else None, hi if clip else None, out.win, act, clip=clip)
        COUNTS['calls'] += 1
        what = f'hrl_llc_action n {n} act {act} pitch {pitch} clip {clip}'
        out.check(what)
        same(out.win, ref_llc_action(mu, low, high, clip), what)
    return mu, low, high


# ---- hrl_accum -----------------------------------------------------------------------------------------------------------------
def flag_sequence(n, T, gen):
    """T flag vectors [n] of 0 / 1: rows 0-7 set in no step, 8-15 in exactly one (which one varies), 16-23 in all, the rest
    at random (where n leaves room)."""
    f = (torch.rand(T, n, generator=gen) < 0.3).to(torch.int64)
    rows = torch.arange(n)
    for lo, kind in ((0, 'none'), (8, 'one'), (16, 'all')):
        sel = rows[lo:lo + 8]
        if sel.numel() == 0:
            continue
        f[:, sel] = 1 if kind == 'all' else 0
        if kind == 'one':
            f[sel % T, sel] = 1
    return f


def accum_case(n, T, gen, ld_l=1):
    rewards = torch.randn(T, n, generator=gen)
    dones, terminate = flag_sequence(n, T, gen), flag_sequence(n, T, gen)
    # logits over [-30, 30], both sides of the 1 - prob = 1e-4 clamp (l = ln 9999 = 9.2102...)
    logit = torch.full((T, n, ld_l), NAN)
    l0 = torch.rand(T, n, generator=gen) * 60.0 - 30.0
    k = min(n, 6)
    l0[:, :k] = torch.tensor([-30.0, 30.0, 9.0, 9.5, 9.2102, 9.2104])[:k]
    logit[:, :, 0] = l0
    return rewards, dones, terminate, logit


def check_accum(be, dev, n, T, dones_dtype=torch.uint8, term_dtype=torch.bool, ld_l=1, seed=9, groups=('terminate', 'logit'),
                case=None, dirty=True):
    """One llc_steps sequence: after every call the accumulator rows bitwise the f32 reference's partial sums, the outputs
    untouched before the last call and bitwise after it; disc_out against f64 at the bar of the module docstring.  The first
    call finds a dirty accumulator (NaN and garbage)."""
    gen = torch.Generator().manual_seed(seed + 31 * n + T)
    rewards, dones, terminate, logit = case if case is not None else accum_case(n, T, gen, ld_l)
    has_t, has_l = 'terminate' in groups, 'logit' in groups
    acc = Guarded((4, n), F32, dev, pad=(1, 3))
    if dirty:
        acc.win.copy_(torch.randn(4, n) * 1e3)
        acc.win[:, ::2] = NAN
        acc.before = acc.alloc.clone()
    outs = {k: vec(n, F32, dev) for k in ('rewards_out', 'disc_out', 'dones_out', 'terminate_out')}
    used = ['rewards_out', 'dones_out'] + (['disc_out'] if has_l else []) + (['terminate_out'] if has_t else [])
    typed = lambda f, dt: f.to(dt).to(dev)
    disc_steps, disc64, disc32 = [], [], []
    what = f'hrl_accum n {n} T {T} kinds {dones_dtype} {term_dtype} ld_l {logit.shape[-1]} groups {groups}'
    acc_before = acc.win.clone()
    for t in range(T):
        lg = logit[t].to(dev)
        if has_l:
            r = torch.empty(n, 1, dtype=F32, device=dev)
            be.disc_reward(lg, r, n, DISC_SCALE)            # the device's own rewards on the same logits, carried to the CPU
            disc_steps.append(r.view(-1).cpu())
            disc64.append(RR.disc_reward(logit[t, :, 0], DISC_SCALE, F64))
            disc32.append(RR.disc_reward(logit[t, :, 0], DISC_SCALE, F32))
        kw = {k: outs[k].win for k in used}
        be.hrl_accum(rewards[t].to(dev), typed(dones[t], dones_dtype), acc.win, t == 0, t == T - 1, T,
                     terminate=typed(terminate[t], term_dtype) if has_t else None, logit=lg if has_l else None,
                     disc_scale=DISC_SCALE, **kw)
        COUNTS['calls'] += 1
        fl = lambda f, dt: [x.to(dt).to(F32) for x in f[:t + 1]]
        partials, finals = ref_fold(list(rewards[:t + 1]), fl(dones, dones_dtype), fl(terminate, term_dtype) if has_t else None,
                                    disc_steps if has_l else None, t + 1)
        acc.check(f'{what} step {t}')
        got = acc.win.cpu()
        for row, p in enumerate(partials[-1]):
            if p is not None:
                same(got[row], p, f'{what} step {t} accumulator row {row}')
            else:
                same(got[row], acc_before[row], f'{what} step {t} untouched accumulator row {row}')
        for k, g in outs.items():
            if t < T - 1 or k not in used:
                g.check(f'{what} step {t} {k} untouched', written=False)
    _, finals = ref_fold(list(rewards), [x.to(dones_dtype).to(F32) for x in dones],
                         [x.to(term_dtype).to(F32) for x in terminate] if has_t else None, disc_steps if has_l else None, T)
    for k, want in zip(('rewards_out', 'disc_out', 'dones_out', 'terminate_out'), finals):
        if want is not None:
            outs[k].check(f'{what} {k}')
            same(outs[k].win, want, f'{what} {k}')
    if has_l:
        mean64 = torch.stack(disc64).sum(0) / T
        a_t = [RR.allowance(d32, d64) for d32, d64 in zip(disc32, disc64)]
        tol = sum(a_t) / T + (T + 1) * 2.0 ** -24 * float(mean64.abs().max())
        err = float((outs['disc_out'].win.cpu().double() - mean64).abs().max())
        STATS['disc_out |got - f64|'] = max(STATS['disc_out |got - f64|'], err)
        STATS['disc_out allowance'] = max(STATS['disc_out allowance'], tol)
        print(f'{what}: disc_out max |got - f64| = {err:.3g}, allowance {tol:.3g}')
        assert err <= tol, (what, err, tol)
    return outs, acc


def special_accum_case(n, T, gen):
    """NaN / +-inf rewards and an f32 flag vector with a NaN and a 0.5."""
    rewards, dones, terminate, logit = accum_case(n, T, gen)
    rewards[0, 0], rewards[0, 1], rewards[T - 1, 2], rewards[0, 3] = NAN, INF, -INF, -0.0
    if T > 1:
        rewards[1, 1] = -INF                   # inf - inf
    dones = dones.to(F32)
    dones[0, 4], dones[T - 1, 5] = NAN, 0.5
    dones[:, 5][:T - 1] = 0.0
    return rewards, dones, terminate, logit


# ---- the inner loop under functions that raise ---------------------------------------------------------------------------------
class InnerLoopGuard:
    """While an agent's (player's) env_step runs - the environment's own step left out - normalize_rows, gather_rows and
    rms_finalize of the backend classes and torch.clamp called from the package raise."""

    def __init__(self, monkeypatch, owner, env, backends):
        self.active = False
        guard = self
        for cls in {type(b) for b in backends}:
            for name in ('normalize_rows', 'gather_rows', 'rms_finalize'):
                orig = getattr(cls, name)

                def wrapper(be, *a, _orig=orig, _name=name, **kw):
                    caller = sys._getframe(1).f_globals.get('__name__', '')           # (a stand-in may use its own row code)
                    assert not (guard.active and caller.startswith('ase_amd')), f'{_name} called inside the inner loop by {caller}'
                    return _orig(be, *a, **kw)
                monkeypatch.setattr(cls, name, wrapper)
        clamp = torch.clamp

        def clamp_wrapper(*a, **kw):
            caller = sys._getframe(1).f_globals.get('__name__', '')
            assert not (guard.active and caller.startswith('ase_amd')), f'torch.clamp called inside the inner loop by {caller}'
            return clamp(*a, **kw)
        monkeypatch.setattr(torch, 'clamp', clamp_wrapper)
        env_step, step = owner.env_step, env.step

        def guarded_env_step(*a, **kw):
            guard.active = True
            try:
                return env_step(*a, **kw)
            finally:
                guard.active = False

        def free_step(actions):
            was, guard.active = guard.active, False
            try:
                return step(actions)
            finally:
                guard.active = was
        monkeypatch.setattr(owner, 'env_step', guarded_env_step)
        monkeypatch.setattr(env, 'step', free_step)


def report():
    return {'counts': dict(COUNTS), 'maxima': dict(STATS)}
