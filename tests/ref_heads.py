"""Plain CPU reference of the loss-head kernels (csrc/heads.hip) - TEST INFRASTRUCTURE ONLY.

Every operation is written from the reference's own FORWARD expressions with a ``dtype`` argument (f32 or f64); every gradient
comes from torch.autograd, never from an analytic formula - tests/emu_backend.py transcribes the kernels' analytic gradients by
the same hand as the kernels, so the two share their mistakes; this file shares none of them.

  learning/common_agent.py:505-519 _actor_loss, :521-534 _critic_loss, :456-464 bound_loss (restated.bound_loss)
  learning/ase_agent.py:237-241,252-258 the masked means and the total, :445-467 _diversity_loss, :413-418,469-472 _enc_loss /
      _calc_enc_error, :431-441 the encoder gradient penalty
  learning/amp_agent.py:442-446,481-489 _disc_loss_neg / _disc_loss_pos (torch.nn.BCEWithLogitsLoss), :491-496 _compute_disc_acc,
      :453-459 the gradient penalty's chain
  rl_games neglogp / policy_kl / Normal entropy (restated.neglogp, restated.policy_kl)

The rule (as tests/ref_rollout.py): max |got - f64| <= 2 e_ref + floor with e_ref = max |f32 run - f64 run| of
THIS reference on the same inputs.  The outputs here carry 1 / M, so the floor is one f32 ulp of the tensor's largest reference
magnitude, 2^-23 max |ref64| (the project's 1e-7 at magnitude 1, rescaled); 16-bit storage adds half an ulp of the storage type,
elementwise, and the comparison is made in the scaled (stored) domain.  Sums and bias gradients have bounds of their own below.

The input cases of tests/test_gpu_heads.py are built here, and one body per operation checks a backend: tests/test_heads_ref.py
runs the emulator over the same cases on the CPU.  No project imports beyond oracle.restated (the slot numbers of
include/ase_hip.h are restated below and compared with ase_amd.lib by tests/test_heads_ref.py)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import restated as R

F32, F64 = torch.float32, torch.float64
NAN = float('nan')
LS_FROZEN, LS_VECTOR, LS_ROWS = 0, 1, 2
ACT_RELU, ACT_TANH, ACT_SILU, ACT_ELU, ACT_GELU, ACT_SIGMOID, ACT_SELU, ACT_SOFTPLUS = range(1, 9)
ACC = {n: i for i, n in enumerate(
    ('MASK_SUM', 'A_LOSS', 'B_LOSS', 'ENTROPY', 'CLIPPED', 'C_LOSS', 'KL', 'DIV', 'BCE_AGENT', 'BCE_DEMO', 'AGENT_ACC', 'DEMO_ACC',
     'GP', 'ENC', 'ENC_GP', 'LOGIT_W2', 'DISC_W2', 'ENC_W2', 'GRAD_SQ'))}
ACC_COUNT = 24
RES = {n: i for i, n in enumerate(
    ('A_LOSS', 'C_LOSS', 'B_LOSS', 'ENTROPY', 'CLIP_FRAC', 'KL', 'DISC_LOSS', 'DISC_GP', 'DISC_LOGIT_LOSS', 'DISC_AGENT_ACC',
     'DISC_DEMO_ACC', 'ENC_LOSS', 'DIV_LOSS', 'LOSS', 'MASK_SUM', 'ENC_GP', 'LR'))}
RES_COUNT = 20
ACC0 = 0.5           # what every accumulator slot holds before a launch ('+=' is checked); exactly representable
DB0 = 0.25           # the same for the bias gradients
MARGIN = 1e-3


def f32(x):
    """A Python float as the f32 value the C entry receives."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ the bounds
STATS = {}           # (operation, output, storage) -> [max err, max e_ref, elements, comparisons]; for COVERAGE.md


def _note(key, err, e_ref, n):
    s = STATS.setdefault(key, [0.0, 0.0, 0, 0])
    s[0], s[1], s[2], s[3] = max(s[0], err), max(s[1], e_ref), s[2] + n, s[3] + 1


def _name(storage):
    return {None: 'f32', torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}[storage]


def half_ulp(x, storage):
    """Half an ulp of the storage type at |x| (elementwise, f64): bf16 has 8 significant bits, IEEE half 11 and subnormals
    below 2^-14.  0 for f32 storage: the f32 rounding is part of e_ref and the floor."""
    if storage in (None, torch.float32):
        return torch.zeros_like(x)
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-300)))
    if storage == torch.float16:
        return torch.exp2(e.clamp_min(-14.0) - 11.0)
    return torch.exp2(e.clamp_min(-126.0) - 8.0)


def within(got, ref64, ref32, name, gs=1.0, storage=None, key=None, extra=None):
    """max |got - gs ref64| <= 2 gs e_ref + 2^-23 max |gs ref64| (+ half a storage ulp at |gs ref64| + that allowance,
    elementwise), in the scaled domain: `got` is what was stored.  Non-finite entries are equal as such.  IEEE half saturates
    (include/ase_hip.h: 'conversions saturate'): the expectation is clamped to +-65504.  Prints both numbers; returns them
    divided by gs.  extra: a further elementwise allowance (unscaled) that the caller derives."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    r64, r32 = ref64.detach().double() * gs, ref32.detach().double() * gs
    if storage == torch.float16:
        r64, r32 = r64.clamp(-65504.0, 65504.0), r32.clamp(-65504.0, 65504.0)
    assert torch.equal(torch.isnan(r32), torch.isnan(r64)), (name, 'the reference disagrees with itself on NaN')
    assert torch.equal(torch.isnan(got), torch.isnan(r64)), (name, 'NaN entries differ', int(torch.isnan(got).sum()), int(torch.isnan(r64).sum()))
    fin = torch.isfinite(r64)
    inf = ~fin & ~torch.isnan(r64)
    assert torch.equal(got[inf], r64[inf]), (name, 'infinite entries differ')
    if not fin.any():
        return 0.0, 0.0
    d = (r32 - r64).abs()
    e_ref = float(d[fin & torch.isfinite(d)].max()) if (fin & torch.isfinite(d)).any() else 0.0
    base = 2 * e_ref + 2.0 ** -23 * float(r64[fin].abs().max())
    if extra is not None:
        base = base + gs * torch.nan_to_num(extra.detach().double())
    tol = base + half_ulp(r64.abs() + base, storage)
    base = float(torch.as_tensor(base).max())
    err_t = (got - r64).abs()
    err = float(err_t[fin].max())
    print(f'{name}: max |got - f64| = {err / gs:.3g}, e_ref = {e_ref / gs:.3g}, allowance {base / gs:.3g} [{_name(storage)}]')
    bad = fin & ~(err_t <= tol)
    if storage == torch.float16:                       # past 65504 (1 + 1e-3) the stored element IS +-65504
        over = fin & ((ref64.detach().double() * gs).abs() > 65504.0 * (1 + 1e-3))
        assert torch.equal(got[over], r64[over]), (name, 'not saturated at +-65504')
    assert not bad.any(), (name, _name(storage), 'elements over the bound', int(bad.sum()), err / gs, base / gs,
                           bad.nonzero()[:4].tolist())
    if key:
        _note(key + (_name(storage),), err / gs, e_ref / gs, int(fin.sum()))
    return err / gs, e_ref / gs


def sum_within(got, terms64, terms32, name, key=None):
    """An accumulator slot: an f64 sum of per-row f32 terms.  |got - sum f64 terms| <= 2 sum_rows |f32 term - f64 term| +
    n 2^-24 max |term| (every f32 term is allowed twice the reference's own f32 error, plus half an f32 ulp of the largest for
    the order of the kernel's own f32 operations) + the f64 roundings of the additions, 4 2^-53 (|sum| + ACC0).  NaN where the
    reference's sum is NaN."""
    t64, t32 = terms64.detach().double().reshape(-1), terms32.detach().double().reshape(-1)
    want = float(t64.sum())
    got = float(got)
    if want != want:
        assert float(t32.sum()) != float(t32.sum()), (name, 'the reference disagrees with itself on NaN')
        assert got != got, (name, 'the sum must be NaN', got)
        return 0.0, 0.0
    n = t64.numel()
    tol = 2 * float((t32 - t64).abs().sum()) + n * 2.0 ** -24 * float(t64.abs().max()) + 4 * 2.0 ** -53 * (abs(want) + ACC0)
    err = abs(got - want)
    print(f'{name}: |sum - f64| = {err:.3g}, allowance {tol:.3g} (n = {n})')
    assert err <= tol, (name, got, want, err, tol)
    if key:
        _note(key + ('f64',), err, float((t32 - t64).abs().sum()), n)
    return err, tol


def bias_within(got, stored, scale, depth, name, db0=DB0, key=None):
    """A bias gradient by its contract (include/ase_hip.h): the column sums of what was STORED, divided by the scale.  `stored`
    [rows, cols] is the output read back, `got` [cols] the bias gradient that started from db0.  Allowed: depth 2^-24 (sum
    |stored term| / scale + |db0|), depth = the f32 additions / roundings on the longest path of that kernel's reduction (each
    rounds at half an ulp of a partial sum no larger than the sum of the magnitudes); the fold between them is f64.  A column
    with a NaN stored element must be NaN."""
    st = stored.detach().double().cpu()
    st = st.reshape(st.shape[0], -1)
    want = st.sum(0) / scale + db0
    got = got.detach().double().cpu().reshape(-1)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (name, 'NaN columns differ')
    if nan.all():
        return 0.0
    tol = depth * 2.0 ** -24 * (st.abs().sum(0) / scale + abs(db0))
    err = (got - want).abs()
    print(f'{name}: max |db - column sum of the stored| = {float(err[~nan].max()):.3g}, allowance {float(tol[~nan].max()):.3g} '
          f'(depth {depth})')
    assert bool((err[~nan] <= tol[~nan]).all()), (name, float(err[~nan].max()), float(tol[~nan].max()))
    if key:
        _note(key + ('f32',), float(err[~nan].max()), 0.0, int((~nan).sum()))
    return float(err[~nan].max())


# ------------------------------------------------------------------------------------------------ the PPO head
def ppo_head(c, dtype=F64):
    """The loss of one minibatch as the reference forms it, and its autograd gradients.  c: a case of ppo_case().
    m_global, mask_sum (the GLOBAL mask sum in acc[MASK_SUM]) are arguments of their own: a rank's rows are a part of the batch.
    Returns d_mu [R, A] (both row blocks with diversity), d_value [M], d_logstd [M, A] (per row, learned modes; the vector's
    gradient is its column sum), mu_out, the per-row terms of the seven accumulator slots, and the branch quantities."""
    M, A = c['M'], c['A']
    e_clip, cc, bc, dc, dt_, ec = (f32(c[k]) for k in ('e_clip', 'critic_coef', 'bounds_coef', 'div_coef', 'div_tar', 'entropy_coef'))
    t = lambda x: x.to(dtype)
    mu = t(c['mu']).clone().requires_grad_(True)
    value = t(c['value']).clone().requires_grad_(True)
    learned = c['ls_mode'] != LS_FROZEN
    ls = t(c['logstd'])
    lsr = (ls if ls.dim() == 2 else ls.expand(M, A)).clone().requires_grad_(learned)
    mm = torch.tanh(mu) if c['mu_tanh'] else mu                     # learning/hrl_network_builder.py:26-29
    m = mm[:M]
    sg = torch.exp(lsr)
    nlp = R.neglogp(t(c['actions']), m, sg, lsr)
    # learning/common_agent.py:505-519
    ratio = torch.exp(t(c['old_logp']) - nlp)
    adv = t(c['adv'])
    surr1 = adv * ratio
    surr2 = adv * torch.clamp(ratio, 1.0 - e_clip, 1.0 + e_clip)
    a_loss = torch.max(-surr1, -surr2)
    clipped = (torch.abs(ratio - 1.0) > e_clip).to(dtype)
    # learning/common_agent.py:521-534
    ret = t(c['returns'])
    dlt = None
    if c['clip_value']:
        ov = t(c['old_values'])
        dlt = value - ov
        vpc = ov + dlt.clamp(-e_clip, e_clip)
        c_loss = torch.max((value - ret) ** 2, (vpc - ret) ** 2)
    else:
        c_loss = (ret - value) ** 2
    b_loss = R.bound_loss(m)
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + lsr).sum(-1)       # torch.distributions.Normal(mu, sigma).entropy().sum(-1)
    # restated.policy_kl(p0 = new, p1 = old) per row (its .mean() is ACC_KL / m_global); sigma detached (ase_agent.py:290-292)
    sgd, omu, osg = sg.detach(), t(c['old_mu']), t(c['old_sigma'])
    kl = (torch.log(osg / sgd + 1e-5) + (sgd ** 2 + (omu - m.detach()) ** 2) / (2.0 * (osg ** 2 + 1e-5)) - 0.5).sum(-1)
    mk = t(c['mask']) if c['masked'] else torch.ones(M, dtype=dtype)
    S = float(c['mask_sum']) if c['masked'] else float(c['m_global'])            # ase_agent.py:237-241 / torch.mean
    loss = (mk * a_loss).sum() / S + cc * c_loss.sum() / c['m_global'] + bc * (mk * b_loss).sum() / S - ec * (mk * ent).sum() / S
    div = torch.zeros(M, dtype=dtype)
    m2 = None
    if c['div_on']:
        # learning/ase_agent.py:445-467, :255-258
        m2 = mm[M:]
        a_diff = torch.mean(torch.square(torch.clamp(m, -1.0, 1.0) - torch.clamp(m2, -1.0, 1.0)), dim=-1)
        z_diff = 0.5 - 0.5 * torch.sum(t(c['new_z']) * t(c['z']), dim=-1)
        div = torch.square(dt_ - a_diff / (z_diff + 1e-5))
        loss = loss + dc * (mk * div).sum() / S
    # What the floor does not cover: ratio = exp(old_logp - nlp) takes the exponential of a difference of numbers of magnitude
    # |nlp| (tens, for tens of actions), so every f32 rounding at that magnitude - half an ulp, 2^-24 cond with cond = 0.5 sum d^2
    # + 0.5 ln(2 pi) A + sum |logstd| + |old_logp| - is a RELATIVE error of the same size in ratio and in the surrogate's
    # gradient.  Counted from ppo_head_kernel: 6 additions of the butterfly over a row's lanes, 3 relative roundings per
    # element of d^2 (subtraction, division, square; their sum is bounded by sum d^2), the 2 additions that form nlp and the
    # subtraction from old_logp: 12.  The allowance is 12 2^-24 cond |surrogate part of the gradient|, per element.
    sur = (mk * a_loss).sum() / S
    g_mu = torch.autograd.grad(sur, mu, retain_graph=True)[0].detach()
    g_ls = torch.autograd.grad(sur, lsr, retain_graph=True)[0].detach() if learned else None
    cond = (0.5 * (((t(c['actions']) - m) / sg) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * A + lsr.abs().sum(-1)
            + t(c['old_logp']).abs()).detach().view(-1, 1)
    x_mu = torch.zeros_like(g_mu)
    x_mu[:M] = 12 * 2.0 ** -24 * cond * g_mu[:M].abs()
    x_ls = 12 * 2.0 ** -24 * cond * g_ls.abs() if learned else None
    loss.backward()
    terms = {'A_LOSS': mk * a_loss, 'B_LOSS': mk * b_loss, 'ENTROPY': mk * ent, 'CLIPPED': mk * clipped, 'C_LOSS': c_loss,
             'KL': kl, 'DIV': mk * div}
    return {'d_mu': mu.grad, 'd_value': value.grad, 'd_logstd': lsr.grad if learned else None, 'mu_out': m.detach(),
            'x_mu': x_mu, 'x_ls': x_ls, 'terms': {k: v.detach() for k, v in terms.items()}, 'ratio': ratio.detach(), 'adv': adv,
            'dlt': None if dlt is None else dlt.detach(), 'm': m.detach(), 'm2': None if m2 is None else m2.detach()}


def _ppo_draw(n, A, Z, g):
    r = lambda *s: torch.randn(*s, generator=g)
    mu = r(n, A) * 0.8
    old_mu = mu + 0.05 * r(n, A)
    old_sigma = torch.exp(-1.0 + 0.3 * r(n, A))
    actions = old_mu + old_sigma * r(n, A)
    noise = 0.25 * r(n)
    old_values = r(n)
    z = F.normalize(r(n, max(Z, 1)), dim=-1)
    return {'mu': mu, 'mu2': mu + 0.5 * r(n, A), 'old_mu': old_mu, 'old_sigma': old_sigma, 'actions': actions, 'noise': noise,
            'adv': r(n), 'old_values': old_values, 'value': old_values + 0.4 * r(n), 'returns': r(n), 'z': z,
            'new_z': F.normalize(r(n, max(Z, 1)), dim=-1), 'ls_rows': -1.0 + 0.3 * r(n, A)}


def ppo_margins(c, out):
    """Per row: True where a branch quantity of the f64 run is closer than MARGIN to its threshold (exact ties excepted)."""
    e = f32(c['e_clip'])
    ratio = out['ratio']
    bad = ((ratio - (1 + e)).abs() < MARGIN) | ((ratio - (1 - e)).abs() < MARGIN) | (((ratio - 1).abs() - e).abs() < MARGIN)
    if out['dlt'] is not None:
        bad |= ((out['dlt'].abs() - e).abs() < MARGIN) & ~c['tie_v']
    near = lambda m: (((m.abs() - 1).abs() < MARGIN) & (m.abs() != 1.0)).any(-1)
    bad |= near(out['m'])
    if out['m2'] is not None:
        bad |= near(out['m2'])
    return bad


def ppo_case(M, A, m_global=None, masked='off', Z=0, mu_tanh=False, clip_value=False, ls_mode=LS_FROZEN, ec=0.0, ties=False,
             nan_row=None, seed=0):
    """One input case.  masked: 'off' / 'random' / 'one' (exactly one row set) / 'ones'.  Z > 0 turns the diversity loss on;
    every fifth row then has new_z == z == a unit vector of the basis, so z . new_z is exactly 1 in any precision and order
    (z_diff = 0; mu2 close to mu there, or the bonus a_diff / 1e-5 would dwarf every other row).  Rows closer than MARGIN to a
    branch threshold in the f64 run are drawn again.  ties (e_clip 0.25, M >= 8, no tanh): rows 0..3, 5 and 6 hold the exactly
    representable ties of the issue."""
    g = torch.Generator().manual_seed(1000 * M + 10 * A + seed)
    div_on = Z > 0
    d = _ppo_draw(M, A, Z, g)
    ls_vec = -1.0 + 0.3 * torch.randn(A, generator=g)
    e_clip = 0.25 if ties else 0.2
    c = {'M': M, 'A': A, 'Z': Z, 'm_global': M if m_global is None else m_global, 'masked': masked != 'off', 'div_on': div_on,
         'mu_tanh': mu_tanh, 'clip_value': clip_value, 'ls_mode': ls_mode, 'e_clip': e_clip, 'critic_coef': 5.0,
         'bounds_coef': 10.0, 'div_coef': 0.01, 'div_tar': 1.0, 'entropy_coef': ec, 'nan_row': nan_row, 'ties': ties,
         'name': f'M{M} A{A} mg{m_global or M} mask={masked} Z{Z} tanh={int(mu_tanh)} clipv={int(clip_value)} ls{ls_mode} '
                 f'ec{ec:g} ties={int(ties)} nan={nan_row}'}
    mask = torch.ones(M)
    if masked == 'random':
        mask = (torch.rand(M, generator=g) < 0.7).float()
        mask[0] = 1.0
    elif masked == 'one':
        mask = torch.zeros(M)
        mask[M // 2] = 1.0
    if ties and masked != 'off':
        mask[:7] = 1.0                                     # the tie rows take part
    c['mask'] = mask
    c['mask_sum'] = float(mask.sum()) + (c['m_global'] - M) // 2          # the other ranks' rows
    tie_v = torch.zeros(M, dtype=torch.bool)

    def assemble():
        c['logstd'] = d['ls_rows'] if ls_mode == LS_ROWS else ls_vec
        c['mu'] = torch.cat([d['mu'], d['mu2']]) if div_on else d['mu']
        for k in ('old_mu', 'old_sigma', 'actions', 'adv', 'old_values', 'value', 'returns', 'z', 'new_z'):
            c[k] = d[k]
        ls = c['logstd'] if ls_mode == LS_ROWS else ls_vec.expand(M, A)
        m = torch.tanh(d['mu']) if mu_tanh else d['mu']
        c['old_logp'] = (R.neglogp(d['actions'].double(), m.double(), torch.exp(ls.double()), ls.double()) + d['noise'].double()).float()

    def special(rows):
        if div_on:
            k = rows[rows % 5 == 4]
            e = torch.zeros(len(k), Z)
            e[torch.arange(len(k)), k % Z] = 1.0
            d['z'][k], d['new_z'][k] = e, e.clone()
            d['mu2'][k] = d['mu'][k] + 0.003 * torch.randn(len(k), A, generator=g)
        if ties:
            assert M >= 8 and not mu_tanh and e_clip == 0.25
            d['adv'][0] = 0.0
            d['value'][1] = d['old_values'][1]
            d['old_values'][2], d['value'][2] = 0.5, 0.75
            d['old_values'][3], d['value'][3] = 0.5, 0.25
            d['mu'][5, ::2], d['mu'][6, ::2] = 1.0, -1.0        # (not row 4: a z_diff = 0 row)
            d['mu2'][5, ::3], d['mu2'][6, ::3] = -1.0, 1.0
            tie_v[2:4] = True

    special(torch.arange(M))
    assemble()
    c['tie_v'] = tie_v
    for _ in range(200):
        bad = ppo_margins(c, ppo_head(c))
        if not bad.any():
            break
        idx = bad.nonzero().view(-1)
        fresh = _ppo_draw(len(idx), A, Z, g)
        for k in d:
            d[k][idx] = fresh[k]
        special(torch.arange(M))
        assemble()
    else:
        raise AssertionError('no draw clears the margins: ' + c['name'])
    if nan_row is not None:
        c['mu'] = c['mu'].clone()
        c['mu'][nan_row] = NAN
        if clip_value:                                     # and the value: the clipped critic loss must not swallow it
            c['value'] = c['value'].clone()
            c['value'][nan_row] = NAN
    return c


def ppo_branches(c, out):
    """Rows per branch on the f64 run: the four surrogate branches, the three value-clip branches, mu above 1 / below -1 /
    inside for both row blocks (a row is in a mu branch when one of its elements is)."""
    e, ratio, adv = f32(c['e_clip']), out['ratio'], out['adv']
    n = {'ratio_low': int((ratio < 1 - e).sum()), 'ratio_in_pos': int(((ratio - 1).abs() < e)[adv > 0].sum()),
         'ratio_in_neg': int(((ratio - 1).abs() < e)[adv < 0].sum()), 'ratio_high': int((ratio > 1 + e).sum())}
    if out['dlt'] is not None:
        n.update(v_low=int((out['dlt'] < -e).sum()), v_in=int((out['dlt'].abs() < e).sum()), v_high=int((out['dlt'] > e).sum()))
    for k, m in (('m', out['m']), ('m2', out['m2'])):
        if m is not None and not c['mu_tanh']:
            n.update({k + '_above': int((m > 1).any(-1).sum()), k + '_below': int((m < -1).any(-1).sum()),
                      k + '_inside': int((m.abs() < 1).any(-1).sum())})
    return n


PPO_SHAPES = ((1, 1), (7, 31), (9, 32), (257, 33), (300, 64), (8200, 28), (4100, 64))
PPO_VARIANTS = {'plain': {}, 'masked_div': dict(masked='random', Z=64), 'tanh_clip': dict(mu_tanh=True, clip_value=True),
                'ls_vector': dict(ls_mode=LS_VECTOR, ec=0.01), 'ls_rows': dict(ls_mode=LS_ROWS, ec=0.01, masked='random', Z=64)}


def ppo_option_cases(M, A):
    """Every option, at (257, 33) and (300, 64), f32 storage."""
    out = {}
    for mg in (None, 2 * M + 3):
        for masked in ('off', 'random', 'one', 'ones'):
            out[f'mg{mg}-{masked}'] = dict(m_global=mg, masked=masked, Z=64 if masked in ('off', 'random') else 0)
    for Z in (1, 65):
        out[f'Z{Z}'] = dict(Z=Z, masked='random')
    out['tanh'] = dict(mu_tanh=True, Z=64)
    out['clipv'] = dict(clip_value=True)
    out['ties'] = dict(ties=True, clip_value=True, Z=64)
    out['ties_masked'] = dict(ties=True, clip_value=True, Z=64, masked='random', m_global=2 * M + 3)
    for ls in (LS_VECTOR, LS_ROWS):
        for ec in (0.0, 0.01):
            out[f'ls{ls}-ec{ec:g}'] = dict(ls_mode=ls, ec=ec, Z=64 if ec else 0, masked='random' if ec else 'off')
    if (M, A) == (257, 33):
        out['nan_row'] = dict(nan_row=130, Z=64, clip_value=True)
        out['nan_row_masked'] = dict(nan_row=130, masked='random', ls_mode=LS_ROWS, ec=0.01)
    return {k: (lambda kw=kw: ppo_case(M, A, **kw)) for k, kw in out.items()}


def _ppo_depth(c):
    """f32 roundings on the longest path of ppo_head's bias-gradient reduction: per trip of the row loop one product with
    1 / gs and one addition; the sum of the two row blocks; ROWS additions over the workgroup's rows in LDS; (the slabs fold in
    f64;) one conversion to f32 and one atomic addition per folding workgroup (1 below 64 workgroups, else 8); 1 / gs itself."""
    rows = 8 if c['A'] <= 32 else 4
    grid = min((c['M'] + rows - 1) // rows, 1024)
    trips = (c['M'] + grid * rows - 1) // (grid * rows)
    return 2 * trips + 1 + rows + 1 + (8 if grid >= 64 else 1) + 1


def _nanbuf(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype).to(dev)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def run_ppo_head(b, dev, c, storage, gs=1.0, dyn=None):
    """The launch inside sentinel-filled (NaN) allocations: mu / d_mu are column windows [0, A) of 128-wide head buffers with the
    per-row log-std and its gradient at column 64, the value is column 0 of a 64-wide buffer, one more row after the last.
    Returns what was read back."""
    M, A = c['M'], c['A']
    Rw = c['mu'].shape[0]
    MU = torch.full((Rw + 1, 128), NAN)
    MU[:Rw, :A] = c['mu']
    if c['ls_mode'] == LS_ROWS:
        MU[:M, 64:64 + A] = c['logstd']
    MU = MU.to(dev)
    V = torch.full((M + 1, 64), NAN)
    V[:M, 0] = c['value']
    V = V.to(dev)
    mb = {'actions': c['actions'], 'mu': c['old_mu'], 'sigma': c['old_sigma'], 'old_logp_actions': c['old_logp'].view(M, 1),
          'advantages': c['adv'].view(M, 1), 'old_values': c['old_values'].view(M, 1), 'returns': c['returns'].view(M, 1)}
    if c['masked']:
        mb['rand_action_mask'] = c['mask'].view(M, 1)
    if c['div_on']:
        mb['ase_latents'] = c['z']
    mb = {k: v.contiguous().to(dev) for k, v in mb.items()}
    acc = torch.full((ACC_COUNT,), ACC0, dtype=torch.float64)
    acc[ACC['MASK_SUM']] = c['mask_sum']
    acc = acc.to(dev)
    dMU, dV = _nanbuf((Rw + 1, 128), dev, storage), _nanbuf((M + 1, 64), dev, storage)
    db_mu, db_v, db_ls = (torch.full((n,), DB0).to(dev) for n in (A + 2, 2, A + 2))
    mu_out = _nanbuf((M + 1, A), dev)
    learned = c['ls_mode'] != LS_FROZEN
    kw = {}
    if learned:
        kw = dict(ls_mode=c['ls_mode'], d_logstd=dMU[:, 64:], db_logstd=db_ls, entropy_coef=c['entropy_coef'])
    logstd = MU[:, 64:] if c['ls_mode'] == LS_ROWS else c['logstd'].to(dev)
    b.ppo_head(MU, V, mb, c['new_z'].contiguous().to(dev) if c['div_on'] else None, logstd, dMU, dV, db_mu, db_v, acc, M,
               c['m_global'], A, c['Z'], c['masked'], c['div_on'], c['mu_tanh'], c['clip_value'], c['e_clip'], c['critic_coef'],
               c['bounds_coef'], c['div_coef'], c['div_tar'], mu_out=mu_out, grad_scale=gs, dyn=dyn, **kw)
    if dev != 'cpu':
        torch.cuda.synchronize()
    return {'dMU': dMU.cpu(), 'dV': dV.cpu(), 'db_mu': db_mu.cpu(), 'db_v': db_v.cpu(), 'db_ls': db_ls.cpu(), 'acc': acc.cpu(),
            'mu_out': mu_out.cpu(), 'Rw': Rw}


def ppo_sentinels(c, o):
    M, A, Rw = c['M'], c['A'], o['Rw']
    learned = c['ls_mode'] != LS_FROZEN
    dMU = o['dMU']
    assert _all_nan(dMU[Rw:]) and _all_nan(dMU[:, A:64]) and _all_nan(dMU[:, 64 + A:]), 'd_mu: sentinel overwritten'
    if not learned:
        assert _all_nan(dMU[:, 64:]), 'frozen log-std: columns 64.. belong to nobody'
    assert _all_nan(o['dV'][M:]) and _all_nan(o['dV'][:, 1:]), 'd_value: sentinel overwritten'
    assert _all_nan(o['mu_out'][M:]), 'mu_out: sentinel overwritten'
    assert bool((o['db_mu'][A:] == DB0).all()) and float(o['db_v'][1]) == DB0 and bool((o['db_ls'][A if learned else 0:] == DB0).all())
    used = {ACC[k] for k in ('MASK_SUM', 'A_LOSS', 'B_LOSS', 'ENTROPY', 'CLIPPED', 'C_LOSS', 'KL')} | ({ACC['DIV']} if c['div_on'] else set())
    rest = [i for i in range(ACC_COUNT) if i not in used]
    assert bool((o['acc'][rest] == ACC0).all()) and float(o['acc'][ACC['MASK_SUM']]) == c['mask_sum'], 'foreign accumulator slots'


def check_ppo_head(b, dev, c, storage, who, ref=None):
    """One case on one backend: stored gradients by the bound, loss sums by the sum bound, ACC_CLIPPED exactly, bias gradients
    by their contract, every sentinel.  ref: (f64 run, f32 run), shared between storage types."""
    M, A = c['M'], c['A']
    r64, r32 = ref if ref is not None else (ppo_head(c), ppo_head(c, F32))
    gs = 64.0 if storage == torch.float16 else 1.0
    o = run_ppo_head(b, dev, c, storage, gs)
    ppo_sentinels(c, o)
    Rw, tag, key = o['Rw'], f'{who} ppo_head {c["name"]}', ('ppo_head',)
    nan_row = c['nan_row']
    rows = torch.ones(Rw, dtype=torch.bool)
    if nan_row is not None and storage == torch.float16:
        # include/ase_hip.h says of IEEE half only that its conversions saturate; it says nothing of a NaN that reaches the
        # saturating conversion, so nothing is asserted of the NaN row's stored elements in f16 storage
        rows[nan_row] = False
        if c['div_on']:
            rows[M + nan_row] = False
    elif nan_row is not None:
        assert bool(torch.isnan(r64['d_mu'][nan_row]).all()) and not torch.isfinite(o['dMU'][nan_row, :A].float()).any()
    within(o['dMU'][:Rw, :A][rows], r64['d_mu'][rows], r32['d_mu'][rows], tag + ' d_mu', gs, storage, key + ('d_mu',),
           extra=r64['x_mu'][rows])
    within(o['dV'][:M, 0][rows[:M]], r64['d_value'][rows[:M]], r32['d_value'][rows[:M]], tag + ' d_value', gs, storage, key + ('d_value',))
    if c['ls_mode'] != LS_FROZEN:
        within(o['dMU'][:M, 64:64 + A][rows[:M]], r64['d_logstd'][rows[:M]], r32['d_logstd'][rows[:M]], tag + ' d_logstd', gs,
               storage, key + ('d_logstd',), extra=r64['x_ls'][rows[:M]])
        if c['div_on']:
            assert bool((o['dMU'][M:Rw, 64:64 + A].float() == 0).all()), 'the diversity rows of d_logstd are written as zero'
    if c['mu_tanh']:
        within(o['mu_out'][:M], r64['mu_out'], r32['mu_out'], tag + ' mu_out', key=key + ('mu_out',))
    else:
        assert torch.equal(o['mu_out'][:M].view(torch.int32), c['mu'][:M].view(torch.int32)), 'mu_out is bitwise mu'
    for k in ('A_LOSS', 'B_LOSS', 'ENTROPY', 'C_LOSS', 'KL') + (('DIV',) if c['div_on'] else ()):
        sum_within(float(o['acc'][ACC[k]]) - ACC0, r64['terms'][k], r32['terms'][k], f'{tag} ACC_{k}', key + ('ACC_' + k,))
    assert float(o['acc'][ACC['CLIPPED']]) - ACC0 == float(r64['terms']['CLIPPED'].sum()), 'ACC_CLIPPED'
    assert torch.equal(r64['terms']['CLIPPED'], r32['terms']['CLIPPED'].double())
    if not (nan_row is not None and storage == torch.float16):
        depth = _ppo_depth(c)
        st = o['dMU'][:Rw, :A].double()
        bias_within(o['db_mu'][:A], torch.cat([st[:M], st[M:]], 0) if c['div_on'] else st, gs, depth, tag + ' db_mu', key=key + ('db_mu',))
        bias_within(o['db_v'][:1], o['dV'][:M, :1], gs, depth, tag + ' db_value', key=key + ('db_value',))
        if c['ls_mode'] != LS_FROZEN:
            bias_within(o['db_ls'][:A], o['dMU'][:M, 64:64 + A], gs, depth, tag + ' db_logstd', key=key + ('db_logstd',))
    return o


def check_ppo_record(b, dev, c, storage, who):
    """A record {0.5, 0} with grad_scale g stores bitwise what grad_scale g / 2 stores without one; the count stays bitwise 0."""
    g = 64.0 if storage == torch.float16 else 2.0
    rec = torch.tensor([0.5, 0.0]).to(dev)
    a, p = run_ppo_head(b, dev, c, storage, g, dyn=rec), run_ppo_head(b, dev, c, storage, g / 2)
    for k in ('dMU', 'dV'):
        assert torch.equal(a[k].view(torch.int16 if storage != torch.float32 else torch.int32),
                           p[k].view(torch.int16 if storage != torch.float32 else torch.int32)), k
    assert rec.cpu().view(torch.int32).tolist() == [0x3F000000, 0], 'the count word stays bitwise 0'


def check_ppo_saturation(b, dev, c, who, ref):
    """f16 storage with a grad_scale (a power of two) that carries the largest |d_mu| past 65504: count > 0, the elements past
    65504 (1 + 1e-3) sit at +-65504, everything is within the bound of the clamped expectation."""
    r64, r32 = ref
    big = float(r64['d_mu'].abs().max())
    g = 2.0 ** math.ceil(math.log2(65504.0 * 1.01 / big))
    rec = torch.tensor([1.0, 0.0]).to(dev)
    o = run_ppo_head(b, dev, c, torch.float16, g, dyn=rec)
    ppo_sentinels(c, o)
    assert float(rec.cpu()[1]) > 0, 'a saturated element must be reported'
    got = o['dMU'][:o['Rw'], :c['A']].double()
    over = (r64['d_mu'].abs() * g) > 65504.0 * (1 + 1e-3)
    assert int(over.sum()) >= 1 and torch.equal(got[over], 65504.0 * torch.sign(r64['d_mu'][over]))
    within(got, r64['d_mu'], r32['d_mu'], f'{who} ppo_head saturating d_mu', g, torch.float16, extra=r64['x_mu'])
    within(o['dV'][:c['M'], 0], r64['d_value'], r32['d_value'], f'{who} ppo_head saturating d_value', g, torch.float16)


# ------------------------------------------------------------------------------------------------ the discriminator head
def disc_head(logit, amb, amb_global, disc_coef, dtype=F64):
    """learning/amp_agent.py:442-446,481-496 on the [2 amb agent | amb demo] column; the means are over the GLOBAL batch."""
    l = logit.to(dtype).clone().requires_grad_(True)
    la, ld = l[:2 * amb], l[2 * amb:]
    bce = torch.nn.BCEWithLogitsLoss(reduction='none')
    ta, td = bce(la, torch.zeros_like(la)), bce(ld, torch.ones_like(ld))
    loss = f32(disc_coef) * 0.5 * (ta.sum() / (2 * amb_global) + td.sum() / amb_global)
    loss.backward()
    return {'d_logit': l.grad, 'bce_agent': ta.detach(), 'bce_demo': td.detach(), 'agent_acc': float((la < 0).sum()),
            'demo_acc': float((ld > 0).sum())}


DISC_AMBS = (1, 85, 86, 1000)


def disc_case(amb, amb_global, ld):
    """A grid over [-30, 30]; exactly 0.0 and -0.0 in both blocks (they count for neither accuracy); +-100, where the sigmoid
    saturates, in both blocks; a special value at each edge of the workgroup that 3 x 85 = 255 and 3 x 86 = 258 straddle.
    |logit| >= MARGIN except the exact zeros."""
    n = 3 * amb
    col = torch.linspace(-30, 30, n) if n > 3 else torch.tensor([0.0, -2.5, 100.0])
    col[(col.abs() < MARGIN)] = 0.5
    if amb >= 85:
        for base in (0, 2 * amb):
            col[base + 1], col[base + 2], col[base + 3], col[base + 4] = 0.0, -0.0, 100.0, -100.0
        col[n - 1], col[n - 2], col[255 if n > 255 else n - 3] = -0.0, 100.0, 0.0
    return {'name': f'amb{amb} ag{amb_global} ld{ld}', 'amb': amb, 'amb_global': amb_global, 'ld': ld, 'logit': col, 'disc_coef': 5.0}


def run_disc_head(b, dev, c, storage, gs=1.0, dyn=None):
    amb, ld, n = c['amb'], c['ld'], 3 * c['amb']
    HD = torch.full((n + 1, ld), NAN)
    HD[:n, 0] = c['logit']
    dHD = _nanbuf((n + 1, ld), dev, storage)
    acc = torch.full((ACC_COUNT,), ACC0, dtype=torch.float64).to(dev)
    db = torch.full((2,), DB0).to(dev)
    b.disc_head(HD.to(dev), dHD, db, acc, amb, c['amb_global'], c['disc_coef'], grad_scale=gs, dyn=dyn)
    if dev != 'cpu':
        torch.cuda.synchronize()
    return {'dHD': dHD.cpu(), 'acc': acc.cpu(), 'db': db.cpu()}


def check_disc_head(b, dev, c, storage, who, gs=None, dyn=None):
    amb, n = c['amb'], 3 * c['amb']
    r64, r32 = (disc_head(c['logit'], amb, c['amb_global'], c['disc_coef'], dt) for dt in (F64, F32))
    assert bool(((c['logit'].abs() >= MARGIN) | (c['logit'] == 0)).all())
    gs = (64.0 if storage == torch.float16 else 1.0) if gs is None else gs
    o = run_disc_head(b, dev, c, storage, gs, dyn)
    gs = gs * (1.0 if dyn is None else float(dyn.cpu()[0]))
    tag, key = f'{who} disc_head {c["name"]}', ('disc_head',)
    assert _all_nan(o['dHD'][n:]) and _all_nan(o['dHD'][:, 1:]) and float(o['db'][1]) == DB0
    within(o['dHD'][:n, 0], r64['d_logit'], r32['d_logit'], tag + ' d_logit', gs, storage, key + ('d_logit',))
    sum_within(float(o['acc'][ACC['BCE_AGENT']]) - ACC0, r64['bce_agent'], r32['bce_agent'], tag + ' ACC_BCE_AGENT', key + ('ACC_BCE_AGENT',))
    sum_within(float(o['acc'][ACC['BCE_DEMO']]) - ACC0, r64['bce_demo'], r32['bce_demo'], tag + ' ACC_BCE_DEMO', key + ('ACC_BCE_DEMO',))
    assert float(o['acc'][ACC['AGENT_ACC']]) - ACC0 == r64['agent_acc'] and float(o['acc'][ACC['DEMO_ACC']]) - ACC0 == r64['demo_acc']
    rest = [i for i in range(ACC_COUNT) if i not in (ACC['BCE_AGENT'], ACC['BCE_DEMO'], ACC['AGENT_ACC'], ACC['DEMO_ACC'])]
    assert bool((o['acc'][rest] == ACC0).all())
    # depth: the division by gs, (the workgroup's sum is f64,) one conversion to f32, one atomic addition per workgroup
    bias_within(o['db'][:1], o['dHD'][:n, :1], gs, 2 + (n + 255) // 256, tag + ' db_logit', key=key + ('db_logit',))


# ------------------------------------------------------------------------------------------------ the encoder head and its penalty
def enc_head(e, z, amb_global, enc_coef, dtype=F64):
    """learning/ase_network_builder.py:214-219 (F.normalize, eps 1e-12), learning/ase_agent.py:413-418,469-472."""
    ev = e.to(dtype).clone().requires_grad_(True)
    pred = F.normalize(ev, dim=-1)
    err = -torch.sum(pred * z.to(dtype), dim=-1)
    (f32(enc_coef) * err.sum() / amb_global).backward()
    return {'d_e': ev.grad, 'enc_out': pred.detach(), 'err': err.detach()}


def enc_gp(e, z, du=None, dtype=F64):
    """learning/ase_agent.py:431-441 around the chain: u = d err / d e and, with du, J du with J = d u / d e by a second
    autograd pass.  On the ball |e| < 1e-12 normalize(e) is the linear map e / 1e-12, so J = 0 there; torch's DOUBLE backward of
    `norm` evaluates 0 / 0 at exactly e = 0 (a property of its formula, not of the function), so for J an all-zero row is
    moved to 1e-18 per element (its square is a normal f32 number) - inside the same ball, where the function is the same linear map."""
    ev = e.to(dtype).clone()
    if du is not None:
        ev[(ev == 0).all(-1)] = 1e-18
    ev.requires_grad_(True)
    err = -torch.sum(F.normalize(ev, dim=-1) * z.to(dtype), dim=-1)
    u, = torch.autograd.grad(err.sum(), ev, create_graph=True)
    if du is None:
        return u.detach()
    if not u.requires_grad:                       # every row on the 1e-12 floor: u does not depend on e
        return torch.zeros_like(u)
    jd, = torch.autograd.grad((u * du.to(dtype)).sum(), ev)
    return jd


ENC_SHAPES = ((1, 1), (5, 63), (4, 64), (7, 65), (6, 128), (517, 64), (4100, 8))


def enc_case(rows, dim, special=False, seed=0):
    """e, z, du with different pitches (NaN in the padding).  special (rows >= 4): row 1 all zero, row 2 all 1e-20 (the 1e-12
    floor is active in both), row 3 NaN in its LAST column (the lane + 64 half when dim > 64)."""
    g = torch.Generator().manual_seed(77 * rows + dim + seed)
    e = torch.randn(rows, dim, generator=g) * 3
    z = F.normalize(torch.randn(rows, dim, generator=g), dim=-1)
    du = torch.randn(rows, dim, generator=g) * 0.1
    kinds = torch.zeros(rows, dtype=torch.long)
    if special:
        assert rows >= 4
        e[1], e[2], e[3, dim - 1] = 0.0, 1e-20, NAN
        kinds[1:4] = torch.tensor([1, 1, 2])
    return {'name': f'rows{rows} dim{dim} special={int(special)}', 'rows': rows, 'dim': dim, 'e': e, 'z': z, 'du': du,
            'kinds': kinds, 'special': special, 'amb_global': 3 * rows + 1, 'enc_coef': 5.0}


def _enc_operands(c, dev):
    rows, dim = c['rows'], c['dim']
    HD = torch.full((rows + 1, 64 + dim + 3), NAN)          # the joint head buffer: the logit in column 0, e in columns 64..
    HD[:rows, 64:64 + dim] = c['e']
    Zb = torch.full((rows + 1, dim + 5), NAN)
    Zb[:rows, :dim] = c['z']
    DU = torch.full((rows + 1, dim + 2), NAN)
    DU[:rows, :dim] = c['du']
    return HD.to(dev), Zb.to(dev), DU.to(dev)


def _rowsets(c, storage=None):
    """The comparisons are made per kind of row - ordinary rows, rows on the 1e-12 floor (their gradients are 1e12 times the
    others'), the NaN row - each as a tensor of its own with its own largest magnitude.  No row is left out, but one: of a
    NaN that reaches IEEE half's saturating conversion include/ase_hip.h states nothing, so the NaN row's STORED elements are
    not compared in f16 storage."""
    kinds = ((0, ''), (1, ' floor rows')) + (() if storage == torch.float16 else ((2, ' NaN row'),))
    return [(n, c['kinds'] == k) for k, n in kinds if (c['kinds'] == k).any()]


def check_enc_head(b, dev, c, storage, who, with_out=True, with_db=True, gs=None, dyn=None, ret=False):
    rows, dim = c['rows'], c['dim']
    r64, r32 = (enc_head(c['e'], c['z'], c['amb_global'], c['enc_coef'], dt) for dt in (F64, F32))
    gs = (64.0 if storage == torch.float16 else 1.0) if gs is None else gs
    HD, Zb, _ = _enc_operands(c, dev)
    dHD = _nanbuf((rows + 1, 64 + dim + 1), dev, storage)
    enc_out = _nanbuf((rows + 1, dim), dev) if with_out else None
    db = torch.full((dim + 2,), DB0).to(dev) if with_db else None
    acc = torch.full((ACC_COUNT,), ACC0, dtype=torch.float64).to(dev)
    b.enc_head(HD[:, 64:], Zb, dHD[:, 64:], db, enc_out, acc, rows, c['amb_global'], dim, c['enc_coef'], grad_scale=gs, dyn=dyn)
    if dev != 'cpu':
        torch.cuda.synchronize()
    dHD, acc = dHD.cpu(), acc.cpu()
    if ret:
        return dHD
    gs = gs * (1.0 if dyn is None else float(dyn.cpu()[0]))
    tag, key = f'{who} enc_head {c["name"]}', ('enc_head',)
    assert _all_nan(dHD[rows:]) and _all_nan(dHD[:, :64]) and _all_nan(dHD[:, 64 + dim:])
    if c['special']:
        assert bool(torch.isnan(r64['d_e'][3]).all()) and bool(torch.isnan(r64['enc_out'][3]).all()) and not r64['enc_out'][1].any()
    for n, rs in _rowsets(c, storage):
        within(dHD[:rows, 64:64 + dim][rs], r64['d_e'][rs], r32['d_e'][rs], tag + ' d_e' + n, gs, storage, key + ('d_e' + n,))
    for n, rs in _rowsets(c):
        if with_out:
            within(enc_out.cpu()[:rows][rs], r64['enc_out'][rs], r32['enc_out'][rs], tag + ' enc_out' + n, key=key + ('enc_out' + n,))
    if with_out:
        assert _all_nan(enc_out.cpu()[rows:])
    sum_within(float(acc[ACC['ENC']]) - ACC0, r64['err'], r32['err'], tag + ' ACC_ENC', key + ('ACC_ENC',))
    assert bool((acc[[i for i in range(ACC_COUNT) if i != ACC['ENC']]] == ACC0).all())
    if with_db:
        db = db.cpu()
        assert bool((db[dim:] == DB0).all())
        # depth: per trip of the row loop the division by gs and the addition; 3 additions over the four waves in LDS; one
        # atomic addition per workgroup
        grid = min((rows + 3) // 4, 128)
        trips = (rows + 4 * grid - 1) // (4 * grid)
        bias_within(db[:dim], dHD[:rows, 64:64 + dim], gs, 2 * trips + 3 + grid, tag + ' db_enc', key=key + ('db_enc',))


def check_enc_gp_seed(b, dev, c, storage, who):
    rows, dim, scale = c['rows'], c['dim'], 4.0
    HD, Zb, _ = _enc_operands(c, dev)
    U = _nanbuf((rows + 1, dim + 7), dev, storage)
    b.enc_gp_seed(HD[:, 64:], Zb, U, rows, dim, scale=scale)
    if dev != 'cpu':
        torch.cuda.synchronize()
    U = U.cpu()
    assert _all_nan(U[rows:]) and _all_nan(U[:, dim:])
    r64, r32 = enc_gp(c['e'], c['z']), enc_gp(c['e'], c['z'], dtype=F32)
    for n, rs in _rowsets(c, storage):
        within(U[:rows, :dim][rs], r64[rs], r32[rs], f'{who} enc_gp_seed {c["name"]} u' + n, scale, storage, ('enc_gp_seed', 'u' + n))


def check_enc_gp_back(b, dev, c, storage, who, with_db=True, dyn=None, gs=None, ret=False, old_scale=None):
    rows, dim = c['rows'], c['dim']
    gs = (64.0 if storage == torch.float16 else 1.0) if gs is None else gs
    eff = gs * (1.0 if dyn is None else float(dyn.cpu()[0]))
    HD, Zb, DU = _enc_operands(c, dev)
    g = torch.Generator().manual_seed(5 + rows)
    old = (torch.randn(rows, dim, generator=g) * (0.01 * eff if old_scale is None else old_scale)).to(storage)          # a non-zero d_e, as stored
    left = torch.randn(rows + 1, 64, generator=g).to(storage)
    dHD = torch.full((rows + 1, 64 + dim + 1), NAN, dtype=storage)
    dHD[:, :64] = left
    dHD[:rows, 64:64 + dim] = old
    dHD = dHD.to(dev)
    db = torch.full((dim + 2,), DB0).to(dev) if with_db else None
    b.enc_gp_back(HD[:, 64:], Zb, DU, dHD[:, 64:], db, rows, dim, grad_scale=gs, dyn=dyn)
    if dev != 'cpu':
        torch.cuda.synchronize()
    dHD = dHD.cpu()
    if ret:
        return dHD
    tag, key = f'{who} enc_gp_back {c["name"]}', ('enc_gp_back',)
    bits = torch.int32 if storage == torch.float32 else torch.int16
    assert torch.equal(dHD[:, :64].contiguous().view(bits), left.contiguous().view(bits)), 'the columns before the window'
    assert _all_nan(dHD[rows:, 64:]) and _all_nan(dHD[:, 64 + dim:])
    j64, j32 = enc_gp(c['e'], c['z'], c['du']), enc_gp(c['e'], c['z'], c['du'], F32)
    if c['special']:
        assert not j64[1].any() and not j64[2].any(), 'on the 1e-12 floor u does not depend on e'
    for n, rs in _rowsets(c, storage):
        o64 = old.double()[rs] / eff
        within(dHD[:rows, 64:64 + dim][rs], o64 + j64[rs], o64 + j32[rs].double(), tag + ' d_e' + n, eff, storage, key + ('d_e' + n,))
    if with_db:
        db = db.cpu()
        assert bool((db[dim:] == DB0).all())
        # depth: per trip the subtraction of the old value, the division by the scale and the addition; 3 additions over the
        # four waves; one atomic addition per workgroup
        grid = min((rows + 3) // 4, 128)
        trips = (rows + 4 * grid - 1) // (4 * grid)
        change = dHD[:rows, 64:64 + dim].double() - old.double()
        tol_terms = dHD[:rows, 64:64 + dim].double().abs() + old.double().abs()      # |new| + |old| bounds every partial result
        want = change.sum(0) / eff + DB0
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(db[:dim].double()), nan)
        tol = (3 * trips + 3 + grid) * 2.0 ** -24 * (tol_terms.sum(0) / eff + DB0)
        err = (db[:dim].double() - want).abs()
        if (~nan).any():
            print(f'{tag} db_enc: max |db - column sum of the stored change| = {float(err[~nan].max()):.3g}, allowance {float(tol[~nan].max()):.3g}')
            assert bool((err[~nan] <= tol[~nan]).all()), (tag, float(err[~nan].max()), float(tol[~nan].max()))
            _note(key + ('db_enc', 'f32'), float(err[~nan].max()), 0.0, int((~nan).sum()))


# ------------------------------------------------------------------------------------------------ the penalty chain's pointwise pieces
_ACTS = {ACT_RELU: torch.relu, ACT_TANH: torch.tanh, ACT_SILU: F.silu, ACT_ELU: F.elu, ACT_GELU: F.gelu, ACT_SIGMOID: torch.sigmoid,
         ACT_SELU: F.selu, ACT_SOFTPLUS: F.softplus}


def act_derivs(act, twin, dtype=F64):
    """act'(z), act''(z) by autograd of the activation itself.  The twin is read as the kernel reads it: the activation OUTPUT
    for ReLU (z = h has the same act') and tanh (z = atanh(h)), the PRE-activation z for the others."""
    t = twin.to(dtype)
    z = (torch.atanh(t) if act == ACT_TANH else t).detach().requires_grad_(True)
    d1, = torch.autograd.grad(_ACTS[act](z).sum(), z, create_graph=True)
    d2 = torch.autograd.grad(d1.sum(), z)[0] if d1.requires_grad else torch.zeros_like(d1)
    return d1.detach(), d2


def gp_seed(twin, w, scale, act, dtype=F64):
    """learning/amp_agent.py:453-459: d logit / d pre-activation of the last hidden layer = scale w act'."""
    return f32(scale) * w.to(dtype) * act_derivs(act, twin, dtype)[0]


def gp_second(twin, g, dg, dz, act, dtype=F64):
    """dz + act''(z) u r with u = g / act', r = dg / act' (g = act' u, dg = act' r are the stored chain values); 0 where act'
    vanishes (the chain values are 0 there too)."""
    d1, d2 = act_derivs(act, twin, dtype)
    safe = torch.where(d1 != 0, d1, torch.ones_like(d1))
    term = torch.where(d1 != 0, d2 * (g.to(dtype) / safe) * (dg.to(dtype) / safe), torch.zeros_like(d1))
    return dz.to(dtype) + term


GP_SHAPES = ((1, 1, 1), (3, 513, 513), (200, 512, 576), (1030, 512, 512))          # rows, width, pitch


def gp_case(rows, width, pitch, act, storage):
    g = torch.Generator().manual_seed(rows + width + act)
    z = (torch.randn(rows, width, generator=g) * 1.5).clamp(-3.0, 3.0)
    twin = (_ACTS[act](z) if act in (ACT_RELU, ACT_TANH) else z).to(storage)
    d1 = act_derivs(act, twin.float())[0].float()
    u, r = torch.randn(rows, width, generator=g), torch.randn(rows, width, generator=g)
    return {'name': f'rows{rows} w{width} ld{pitch} act{act}', 'rows': rows, 'width': width, 'pitch': pitch, 'act': act,
            'twin': twin, 'w': torch.randn(width, generator=g), 'g': (d1 * u).to(storage), 'dg': (d1 * r).to(storage),
            'dz': torch.randn(rows, width, generator=g).to(storage)}


def _padded(x, rows, pitch, dev):
    buf = torch.full((rows + 1, pitch + 1), NAN, dtype=x.dtype)
    buf[:rows, :x.shape[1]] = x
    return buf.to(dev)


def check_gp(b, dev, c, storage, who):
    rows, width, pitch, act = c['rows'], c['width'], c['pitch'], c['act']
    tw, G = _padded(c['twin'], rows, pitch, dev), _nanbuf((rows + 1, pitch + 3), dev, storage)
    b.gp_seed(tw, c['w'].to(dev), G, rows, width, scale=0.5, act=act)
    dz = _padded(c['dz'], rows, pitch + 2, dev)
    b.gp_second(tw, _padded(c['g'], rows, pitch, dev), _padded(c['dg'], rows, pitch + 4, dev), dz, rows, width, act)
    if dev != 'cpu':
        torch.cuda.synchronize()
    G, dz = G.cpu(), dz.cpu()
    assert _all_nan(G[rows:]) and _all_nan(G[:, width:]) and _all_nan(dz[rows:]) and _all_nan(dz[:, width:])
    tag = f'{who} {c["name"]}'
    # tanh reads its OUTPUT h and forms act' = 1 - h^2 from a square of magnitude 1: whatever the order of operations, act' is
    # known to no better than one f32 ulp of 1, 2^-23 absolute - a relative 2^-23 / act', which the floor (an ulp of the
    # RESULT's magnitude) does not cover.  It enters gp_seed once (scale w act') and gp_second once (act'' / act' = -2 h is free
    # of it; g / act' is not).
    args = (c['twin'], c['g'], c['dg'], c['dz'], act)
    s64 = gp_second(*args)
    x_seed = x_second = None
    if act == ACT_TANH:
        d1 = act_derivs(act, c['twin'])[0]
        x_seed = 2.0 ** -23 * (0.5 * c['w'].double().abs()).expand(rows, width)
        x_second = 2.0 ** -23 * (s64 - c['dz'].double()).abs() / d1
    within(G[:rows, :width], gp_seed(c['twin'], c['w'], 0.5, act), gp_seed(c['twin'], c['w'], 0.5, act, F32), tag + ' gp_seed', 1.0,
           storage, ('gp_seed', 'g'), extra=x_seed)
    if act == ACT_RELU:
        bits = torch.int32 if storage == torch.float32 else torch.int16
        assert torch.equal(s64, c['dz'].double()) and torch.equal(dz[:rows, :width].contiguous().view(bits), c['dz'].view(bits)), 'gp_second is 0 for ReLU'
    within(dz[:rows, :width], s64, gp_second(*args, F32), tag + ' gp_second', 1.0, storage, ('gp_second', 'dz'), extra=x_second)


# ------------------------------------------------------------------------------------------------ sums
SQNORM_CASES = ((1, 1, 1, 0), (3, 7, 7, 0), (300, 1400, 1408, 0), (300, 1399, 1408, 1))     # rows, cols, pitch, first column


def check_sqnorm(b, dev, rows, cols, pitch, col0, storage, who):
    """Plain f64 sum of the squares of the values as stored, times scale (and the record's factor).  Bound: the kernel squares
    and adds up to 8 elements of a 16-byte chunk in f32 (<= 8 roundings of a partial sum, each half an ulp of at most the
    chunk's sum), the rest is f64: 8 2^-24 sum x^2, times the scale."""
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.full((rows + 1, pitch), NAN, dtype=storage)
    x[:rows, col0:col0 + cols] = torch.randn(rows, cols, generator=g).to(storage)
    xd = x.to(dev)
    for scale, rec in ((1.0, None), (0.375, None), (0.375, torch.tensor([0.5, 0.0]))):
        acc = torch.full((ACC_COUNT,), ACC0, dtype=torch.float64).to(dev)
        recd = None if rec is None else rec.to(dev)
        b.sqnorm(xd[:, col0:], rows, cols, acc, ACC['DISC_W2'], scale=scale, dyn=recd)
        if dev != 'cpu':
            torch.cuda.synchronize()
        acc = acc.cpu()
        eff = scale * (1.0 if rec is None else 0.5)
        sq = float((x[:rows, col0:col0 + cols].double() ** 2).sum())
        err = abs(float(acc[ACC['DISC_W2']]) - ACC0 - eff * sq)
        tol = eff * 8 * 2.0 ** -24 * sq + 4 * 2.0 ** -53 * (ACC0 + eff * sq)
        print(f'{who} sqnorm {rows}x{cols} ld{pitch} +{col0} scale {eff:g} [{_name(storage)}]: |sum - f64| = {err:.3g}, allowance {tol:.3g}')
        assert err <= tol, (err, tol)
        _note(('sqnorm', 'acc', _name(storage)), err / max(eff * sq, 1e-300), 0.0, rows * cols)
        assert bool((acc[[i for i in range(ACC_COUNT) if i != ACC['DISC_W2']]] == ACC0).all())
        if rec is not None:
            assert recd.cpu().view(torch.int32).tolist() == [0x3F000000, 0]


def check_reduce_sum(b, dev, n, square, who):
    """f64 sum of the f32 values (or of their squares, formed in f64): only the f64 additions round."""
    g = torch.Generator().manual_seed(n)
    x = torch.full((n + 3,), NAN)
    x[:n] = torch.randn(n, generator=g) + 0.5
    acc = torch.full((ACC_COUNT,), ACC0, dtype=torch.float64).to(dev)
    b.reduce_sum(x.to(dev), n, square, acc, ACC['MASK_SUM'])
    if dev != 'cpu':
        torch.cuda.synchronize()
    v = x[:n].double()
    want = float((v * v).sum() if square else v.sum())
    mag = float((v * v).sum() if square else v.abs().sum())
    err = abs(float(acc.cpu()[ACC['MASK_SUM']]) - ACC0 - want)
    tol = 2.0 ** -53 * (mag + ACC0) * (math.ceil(math.log2(n + 1)) + 20)      # a tree of f64 additions, generously counted
    print(f'{who} reduce_sum n{n} square={int(square)}: |sum - f64| = {err:.3g}, allowance {tol:.3g}')
    assert err <= tol and bool((acc.cpu()[1:] == ACC0).all()), (err, tol)
    _note(('reduce_sum', 'acc', 'f64'), err / max(mag, 1e-300), 0.0, n)


COLSUM_ROWS = (1, 13, 16, 17, 127, 128, 129, 4096)
COLSUM_COLS = (1, 63, 64, 65, 500)


def check_colsum(b, dev, rows, cols, who, pitch=576, scale=0.25):
    """out[j] += scale * f64 column sum.  depth, counted from colsum_kernel: a workgroup takes 128 rows, 32 per row group,
    8 additions on each of the four chains, 2 to join them, 3 over the row groups in LDS, the product with scale, and one
    atomic addition per 128-row workgroup."""
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.full((rows + 1, pitch), NAN)
    x[:rows, :cols] = torch.randn(rows, cols, generator=g)
    out0 = torch.randn(cols + 5, generator=g)
    out = out0.clone().to(dev)
    b.colsum(x.to(dev), rows, cols, out, scale=scale)
    if dev != 'cpu':
        torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(out[cols:].view(torch.int32), out0[cols:].view(torch.int32)), 'columns past cols are bitwise unchanged'
    want = out0[:cols].double() + scale * x[:rows, :cols].double().sum(0)
    depth = 8 + 2 + 3 + 1 + (rows + 127) // 128
    tol = depth * 2.0 ** -24 * (scale * x[:rows, :cols].double().abs().sum(0) + out0[:cols].double().abs())
    err = (out[:cols].double() - want).abs()
    print(f'{who} colsum {rows}x{cols}: max |out - f64| = {float(err.max()):.3g}, allowance {float(tol.max()):.3g} (depth {depth})')
    assert bool((err <= tol).all()), (float(err.max()), float(tol.max()))
    _note(('colsum', 'out', 'f32'), float(err.max()), 0.0, cols)


# ------------------------------------------------------------------------------------------------ finalize_scalars
FIN_CFG = dict(critic_coef=5, entropy_coef=0.01, bounds_loss_coef=10, disc_coef=5, disc_logit_reg=0.01, disc_grad_penalty=5,
               disc_weight_decay=1e-4, enc_coef=5, enc_weight_decay=1e-3, amp_diversity_bonus=0.01, enc_grad_penalty=3.0)


def finalize(acc, m_global, amb_global, masked, has_disc, has_enc, has_div, cfg, lr=None, kl_threshold=0.0):
    """The arithmetic of ASEAgent.calc_gradients (learning/ase_agent.py:237-258,296-306) / AMPAgent.calc_gradients
    (learning/amp_agent.py:318-333) / CommonAgent.calc_gradients (learning/common_agent.py:386-404) on given sums, in f64,
    with the coefficients as the f32 values the C entry receives.  masked: the masked means divide by the mask sum, else every
    mean - the diversity loss included, as the gradient of ase_hip_ppo_head - divides by m_global.  lr: rl_games
    AdaptiveScheduler.update under the 'legacy' schedule (learning/common_agent.py:204-208), min 1e-6, max 1e-2.
    Returns (RES vector as f64 list, new lr)."""
    a = [float(v) for v in acc]
    k = lambda n: f32(cfg.get(n, 0) or 0.0)
    S = a[ACC['MASK_SUM']]
    den = S if masked else float(m_global)
    out = [0.0] * RES_COUNT
    al, bl, ent, cf = (a[ACC[n]] / den for n in ('A_LOSS', 'B_LOSS', 'ENTROPY', 'CLIPPED'))
    cl, kl = a[ACC['C_LOSS']] / m_global, a[ACC['KL']] / m_global
    loss = al + k('critic_coef') * cl - k('entropy_coef') * ent + k('bounds_loss_coef') * bl
    out[RES['A_LOSS']], out[RES['C_LOSS']], out[RES['B_LOSS']], out[RES['ENTROPY']] = al, cl, bl, ent
    out[RES['CLIP_FRAC']], out[RES['KL']], out[RES['MASK_SUM']] = cf, kl, S
    if has_disc:
        bce = 0.5 * (a[ACC['BCE_AGENT']] / (2.0 * amb_global) + a[ACC['BCE_DEMO']] / amb_global)
        gp = a[ACC['GP']] / amb_global
        dl = bce + k('disc_logit_reg') * a[ACC['LOGIT_W2']] + k('disc_grad_penalty') * gp + k('disc_weight_decay') * a[ACC['DISC_W2']]
        loss += k('disc_coef') * dl
        out[RES['DISC_LOSS']], out[RES['DISC_GP']], out[RES['DISC_LOGIT_LOSS']] = dl, gp, a[ACC['LOGIT_W2']]
        out[RES['DISC_AGENT_ACC']], out[RES['DISC_DEMO_ACC']] = a[ACC['AGENT_ACC']] / (2.0 * amb_global), a[ACC['DEMO_ACC']] / amb_global
    if has_enc:
        egp = a[ACC['ENC_GP']] / amb_global
        el = a[ACC['ENC']] / amb_global + k('enc_weight_decay') * a[ACC['ENC_W2']] + k('enc_grad_penalty') * egp
        loss += k('enc_coef') * el
        out[RES['ENC_LOSS']], out[RES['ENC_GP']] = el, egp
    if has_div:
        dv = a[ACC['DIV']] / den
        loss += k('amp_diversity_bonus') * dv
        out[RES['DIV_LOSS']] = dv
    out[RES['LOSS']] = loss
    new_lr = lr
    if lr is not None:
        out[RES['LR']] = lr
        if kl > 2.0 * f32(kl_threshold):
            new_lr = max(lr / 1.5, 1e-6)
        if kl < 0.5 * f32(kl_threshold):
            new_lr = min(lr * 1.5, 1e-2)
    return out, new_lr


def fin_acc(seed, m_global):
    g = torch.Generator().manual_seed(seed)
    acc = torch.rand(ACC_COUNT, generator=g, dtype=torch.float64) * 50 + 1.0
    acc[ACC['MASK_SUM']] = float(int(0.6 * m_global))
    return acc


def check_finalize(b, dev, acc, m_global, amb_global, masked, has_disc, has_enc, has_div, who, lr=None, kl_threshold=0.0):
    """Every RES slot within one f32 ulp of the f64 arithmetic; slots of absent terms exactly 0; the adapted rate exact up to the
    f64 rounding of one division or product."""
    want, new_lr = finalize(acc, m_global, amb_global, masked, has_disc, has_enc, has_div, FIN_CFG, lr, kl_threshold)
    out = torch.full((RES_COUNT,), NAN).to(dev)
    st = None if lr is None else torch.tensor([0.0, lr, 0.9, 0.999, 1e-8, 1.0, 1.0, 0.0], dtype=torch.float64).to(dev)
    b.finalize_scalars(acc.to(dev), out, m_global, amb_global, masked, has_disc, has_enc, has_div, FIN_CFG, opt_state=st, kl_threshold=kl_threshold)
    if dev != 'cpu':
        torch.cuda.synchronize()
    out = out.cpu().double()
    for n, i in RES.items():
        w = want[i]
        ulp = 2.0 ** (math.floor(math.log2(abs(w))) - 23) if w else 0.0
        assert abs(float(out[i]) - w) <= ulp, (who, 'RES_' + n, float(out[i]), w, ulp)
    absent = ([] if has_disc else ['DISC_LOSS', 'DISC_GP', 'DISC_LOGIT_LOSS', 'DISC_AGENT_ACC', 'DISC_DEMO_ACC']) + \
        ([] if has_enc else ['ENC_LOSS', 'ENC_GP']) + ([] if has_div else ['DIV_LOSS']) + ([] if lr is not None else ['LR'])
    assert all(float(out[RES[n]]) == 0 for n in absent) and bool((out[len(RES):] == 0).all())
    if lr is not None:
        got = float(st.cpu()[1])
        assert abs(got - new_lr) <= 2.0 ** -52 * new_lr, (who, got, new_lr)
    return out


# ------------------------------------------------------------------------------------------------ the plan both test files run
STORAGES = (torch.float32, torch.bfloat16, torch.float16)
_CACHE = {}


def ppo_plan():
    """(id, builder, storage types).  Every option at (257, 33) and (300, 64) in f32; the other shapes and the 16-bit storages
    on the three variants of tests/test_gpu_ops.py::test_ppo_head plus the learned modes; the NaN row in all three."""
    plan = []
    for M, A in ((257, 33), (300, 64)):
        for k, mk in ppo_option_cases(M, A).items():
            plan.append((f'{M}x{A}-{k}', mk, STORAGES if k.startswith('nan_row') else STORAGES[:1]))
    for M, A in PPO_SHAPES:
        for v, kw in PPO_VARIANTS.items():
            plan.append((f'{M}x{A}-{v}', (lambda M=M, A=A, kw=kw: ppo_case(M, A, seed=1, **kw)),
                         STORAGES[1:] if (M, A) in ((257, 33), (300, 64)) else STORAGES))
    return plan


def ppo_get(pid, mk):
    """The case and its two reference runs, computed once and shared among the storage types and the tests."""
    if pid not in _CACHE:
        c = mk()
        _CACHE[pid] = (c, (ppo_head(c), ppo_head(c, F32)))
    return _CACHE[pid]


def disc_plan():
    return [disc_case(amb, ag * amb, ld) for amb in DISC_AMBS for ag in (1, 4) for ld in (1, 128)]


def enc_plan():
    return [enc_case(r, d, sp) for r, d in ENC_SHAPES for sp in ((False, True) if r >= 4 and (r, d) != (4100, 8) else (False,))]


def _pow2_past(big):
    """The power of two that carries `big` past 65504 (1 + 1e-2)."""
    return 2.0 ** math.ceil(math.log2(65504.0 * 1.01 / big))


def check_records(b, dev, storage, who):
    """Scale records on disc_head, enc_head and enc_gp_back: {0.5, 0} with grad_scale g stores bitwise what g / 2 stores without
    a record and the count word stays bitwise 0; in f16 storage a grad_scale that carries the largest element past 65504 gives
    a count > 0, those elements at +-65504 and all others within the bound (within() asserts both)."""
    bits = torch.int32 if storage == torch.float32 else torch.int16
    g = 64.0 if storage == torch.float16 else 2.0
    dc, ec = disc_case(86, 4 * 86, 128), enc_case(517, 64)
    runs = {'disc_head': lambda gs, dyn: run_disc_head(b, dev, dc, storage, gs, dyn)['dHD'],
            'enc_head': lambda gs, dyn: check_enc_head(b, dev, ec, storage, who, gs=gs, dyn=dyn, ret=True),
            'enc_gp_back': lambda gs, dyn: check_enc_gp_back(b, dev, ec, storage, who, gs=gs, dyn=dyn, ret=True, old_scale=0.005 * g)}
    for name, run in runs.items():
        rec = torch.tensor([0.5, 0.0]).to(dev)
        a, p = run(g, rec), run(g / 2, None)
        assert torch.equal(a.contiguous().view(bits), p.contiguous().view(bits)), name
        assert rec.cpu().view(torch.int32).tolist() == [0x3F000000, 0], name
    if storage != torch.float16:
        return
    sat = {'disc_head': (lambda g_, r: check_disc_head(b, dev, dc, storage, who, gs=g_, dyn=r),
                         disc_head(dc['logit'], dc['amb'], dc['amb_global'], dc['disc_coef'])['d_logit']),
           'enc_head': (lambda g_, r: check_enc_head(b, dev, ec, storage, who, gs=g_, dyn=r),
                        enc_head(ec['e'], ec['z'], ec['amb_global'], ec['enc_coef'])['d_e']),
           'enc_gp_back': (lambda g_, r: check_enc_gp_back(b, dev, ec, storage, who, gs=g_, dyn=r, old_scale=1.0),
                           enc_gp(ec['e'], ec['z'], ec['du']))}
    for name, (run, ref) in sat.items():
        rec = torch.tensor([1.0, 0.0]).to(dev)
        g_ = _pow2_past(float(ref.abs().max()))
        assert int(((ref.abs() * g_) > 65504.0 * (1 + 1e-3)).sum()) >= 1
        run(g_, rec)
        assert float(rec.cpu()[1]) > 0, (name, 'a saturated element must be reported')


# ------------------------------------------------------------------------------------------------ tests/test_gpu_learned_sigma.py
# (its inputs and its f64 autograd reference, moved here unchanged)
def _head_inputs(M, A, Z, seed, div_on):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    mu = r(2 * M if div_on else M, A) * 0.6
    ls_rows = -1.0 + 0.3 * r(M, A)
    ls_vec = -1.0 + 0.3 * r(A)
    old_mu = mu[:M] + 0.05 * r(M, A)
    old_sigma = torch.exp(-1.0 + 0.3 * r(M, A))
    actions = old_mu + old_sigma * r(M, A)
    old_logp = (0.5 * (((actions - old_mu) / old_sigma) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * A
                + torch.log(old_sigma).sum(-1) + 0.1 * r(M))
    mb = {'actions': actions, 'mu': old_mu, 'sigma': old_sigma, 'old_logp_actions': old_logp.view(M, 1),
          'advantages': r(M, 1), 'old_values': r(M, 1), 'returns': r(M, 1),
          'rand_action_mask': (torch.rand(M, 1, generator=g) < 0.7).float(),
          'ase_latents': torch.nn.functional.normalize(r(M, Z), dim=-1)}
    new_z = torch.nn.functional.normalize(r(M, Z), dim=-1)
    value = r(M, 1)
    return mu, ls_rows, ls_vec, mb, new_z, value


def _reference(mu, ls, mb, new_z, value, M, A, masked, div_on, mu_tanh, clip_value, e_clip, cc, bc, dc, dt, ec):
    """f64 autograd of the reference's expressions (learning/common_agent.py:456-534, ase_agent.py:228-258,445-467, rl_games
    neglogp / entropy / policy_kl with sigma detached)."""
    mu = mu.double().requires_grad_(True)
    ls = ls.double().requires_grad_(True)
    value = value.double().requires_grad_(True)
    d = {k: v.double() for k, v in mb.items()}
    raw = mu[:M]
    m = torch.tanh(raw) if mu_tanh else raw
    lsr = ls if ls.dim() == 2 else ls.expand(M, A)
    sg = torch.exp(lsr)
    a = d['actions']
    nlp = 0.5 * (((a - m) / sg) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * A + lsr.sum(-1)
    ratio = torch.exp(d['old_logp_actions'].view(-1) - nlp)
    adv = d['advantages'].view(-1)
    a_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - e_clip, 1 + e_clip))
    if clip_value:
        ov = d['old_values'].view(-1)
        vpc = ov + (value.view(-1) - ov).clamp(-e_clip, e_clip)
        c_loss = torch.max((value.view(-1) - d['returns'].view(-1)) ** 2, (vpc - d['returns'].view(-1)) ** 2)
    else:
        c_loss = (d['returns'].view(-1) - value.view(-1)) ** 2
    b_loss = ((m - 1).clamp_min(0) ** 2 + (m + 1).clamp_max(0) ** 2).sum(-1)
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + lsr).sum(-1)
    sgd = sg.detach()
    kl = (torch.log(d['sigma'] / sgd + 1e-5) + (sgd ** 2 + (d['mu'] - m) ** 2) / (2 * (d['sigma'] ** 2 + 1e-5)) - 0.5).sum(-1)
    mk = d['rand_action_mask'].view(-1) if masked else torch.ones(M, dtype=torch.float64)
    mean = lambda x: (x * mk).sum() / mk.sum()
    loss = mean(a_loss) + cc * c_loss.mean() + bc * mean(b_loss) - ec * mean(ent)
    div = torch.zeros((), dtype=torch.float64)
    if div_on:
        raw2 = mu[M:]
        m2 = torch.tanh(raw2) if mu_tanh else raw2
        diff = m.clamp(-1, 1) - m2.clamp(-1, 1)
        a_diff = (diff ** 2).sum(-1) / A
        z_diff = 0.5 - 0.5 * (new_z.double() * d['ase_latents']).sum(-1)
        div = mean((dt - a_diff / (z_diff + 1e-5)) ** 2)
        loss = loss + dc * div
    loss.backward()
    stats = [mean(a_loss), c_loss.mean(), mean(b_loss), mean(ent), mean(((ratio - 1).abs() > e_clip).double()), kl.mean()]
    return torch.stack([s.detach() for s in stats]), mu.grad, ls.grad, value.grad
