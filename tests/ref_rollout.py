"""Plain CPU reference of the rollout kernels (csrc/rollout.hip) - TEST INFRASTRUCTURE ONLY.

Two parts:

* the random draws, stated exactly: Philox4x32-10 (Salmon et al., SC'11) on the counter {elem lo, elem hi, offset lo, offset hi}
  with the key {seed lo, seed hi}, and what the kernels make of its four output words.  THIS FILE IS THE SPECIFICATION of
  the stream: a kernel draws the numbers below or it is wrong.

    normal        Box-Muller on u1 = (f32(c0) + 1) * 2^-32 in (0, 1] and u2 = f32(c1) * 2^-32, both conversions
                  round-to-nearest f32; radius sqrt(-2 ln u1) and cos(6.2831855f * u2) from those f32 uniforms
    keep-uniform  (c2 >> 8) * 2^-24: 24 bits, exact in f32, strictly below 1 (so Bernoulli(1.0) always draws 1)
    elements      sample_actions: normal of (row r, lane) is element r*A + lane, the keep draw of row r is element n*A + r
                  sample_latents: (row_offset + r)*dim + j

* every deterministic operation evaluated from the reference's own formulas (oracle/restated.py, torch.nn.functional.normalize)
  with a ``dtype`` argument, so that a test can form e_ref = max |f32 run - f64 run| on its own inputs and hold the kernel to
  max |hip - f64| <= 2 e_ref + 1e-7.  The input cases of tests/test_gpu_rollout.py are built here as well:
  tests/test_rollout_ref.py runs the emulator (tests/emu_backend.py) over the same cases.

No project imports beyond oracle.restated."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import restated as R

_U64 = (1 << 64) - 1
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
TWO_PI_F32 = np.float32(6.2831855)


# ------------------------------------------------------------------------------------------------ the stream
def philox4x32_10(elem, offset, seed):
    """Four uint32 words per element.  elem: uint64 array (or a non-negative int); offset, seed: Python ints, taken modulo
    2^64 (a negative int64 seed is its two's complement, as the kernel reads the int64 state words)."""
    if isinstance(elem, int):
        elem = elem & _U64
    elem = np.atleast_1d(np.asarray(elem, dtype=np.uint64))
    offset, seed = int(offset) & _U64, int(seed) & _U64
    c = [elem & _LO, elem >> _S32, np.full_like(elem, offset & 0xFFFFFFFF), np.full_like(elem, offset >> 32)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(w.astype(np.uint32) for w in c)


def _box_muller(c0, c1, dtype=np.float64):
    """The normal of two words.  The uniforms are f32 in both runs (they are part of the definition); dtype is the precision
    of log / sqrt / cos and of the product 2 pi * u2."""
    u1 = (c0.astype(np.float32) + np.float32(1)) * np.float32(2.0 ** -32)
    u2 = c1.astype(np.float32) * np.float32(2.0 ** -32)
    if dtype == np.float32:
        return np.sqrt(np.float32(-2) * np.log(u1)) * np.cos(TWO_PI_F32 * u2)
    u1, u2 = u1.astype(np.float64), u2.astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.float64(TWO_PI_F32) * u2)


def keep_uniform(c2):
    return (c2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_uniform_32bit(c2):
    """What the kernel drew before: rounds to exactly 1.0 for every word >= 0xFFFFFF80."""
    return c2.astype(np.float32) * np.float32(2.0 ** -32)


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def normals(elem, offset, seed, dtype=torch.float64):
    w = philox4x32_10(elem, offset, seed)
    return torch.from_numpy(_box_muller(w[0], w[1], _np_dtype(dtype)).reshape(np.shape(elem)))


def latent_elems(rows, dim, row_offset=0):
    r = np.uint64(row_offset) + np.arange(rows, dtype=np.uint64)
    return r[:, None] * np.uint64(dim) + np.arange(dim, dtype=np.uint64)[None, :]


def sample_latents(rows, dim, seed, offset, row_offset=0, dtype=torch.float64):
    """learning/ase_network_builder.py:221-225 on the stream's normals."""
    return F.normalize(normals(latent_elems(rows, dim, row_offset), offset, seed, dtype), dim=-1)


def sample_actions(mu, logstd, rand_probs, seed, offset, n, A, mu_tanh=False, dtype=torch.float64):
    """learning/amp_models.py:29-36 (eval branch) + learning/amp_agent.py:160-166.  mu f32[n, >= A]; logstd f32[A] or
    f32[n, >= A]; rand_probs f32[n] or None.  Returns mu, sigma, sampled, actions, neglogp (dtype) and keep (f32, exact)."""
    m = mu[:n, :A].to(dtype)
    if mu_tanh:
        m = torch.tanh(m)
    ls = (logstd[:A] if logstd.dim() == 1 else logstd[:n, :A]).to(dtype).expand(n, A)
    s = torch.exp(ls)
    r = np.arange(n, dtype=np.uint64)
    a = m + s * normals(r[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :], offset, seed, dtype)
    keep = torch.ones(n)
    if rand_probs is not None:
        u = keep_uniform(philox4x32_10(np.uint64(n) * np.uint64(A) + r, offset, seed)[2])
        keep = torch.from_numpy(u < rand_probs[:n].numpy()).float()
    return {'mu': m, 'sigma': s, 'sampled': a, 'actions': torch.where(keep.view(-1, 1) != 0, a, m),
            'neglogp': R.neglogp(a, m, s, ls), 'keep': keep}


# ------------------------------------------------------------------------------------------------ deterministic operations
def disc_reward(logit, scale, dtype=torch.float64):
    """learning/amp_agent.py _calc_disc_rewards; logit = column 0 of the operand."""
    l = logit.to(dtype)
    prob = 1 / (1 + torch.exp(-l))
    return -torch.log(torch.maximum(1 - prob, torch.tensor(0.0001, dtype=dtype))) * scale


def enc_reward(e, z, scale, dtype=torch.float64):
    """learning/ase_network_builder.py:214-219 (the encoder's normalize) + learning/ase_agent.py:404-411,480-482."""
    pred = F.normalize(e.to(dtype), dim=-1)
    err = -(pred * z.to(dtype)).sum(dim=-1, keepdim=True)
    return (torch.clamp_min(-err, 0.0) * scale).view(-1)


def normalize_rows(x, dtype=torch.float64):
    return F.normalize(x.to(dtype), dim=-1)


def gae(dones, values, next_values, r_task, r_disc, r_enc, w_task, w_disc, w_enc, gamma, tau, dtype=torch.float64):
    """Reward mix (learning/ase_agent.py:95-105) + learning/common_agent.py:437-449; [H, N, 1] operands, dones u8[H, N].
    The entry point rounds gamma and the DOUBLE product gamma * tau to f32; the reference is given those two numbers."""
    g32 = float(np.float32(gamma))
    gt32 = float(np.float32(gamma * tau))
    r = w_task * r_task.to(dtype)
    if r_disc is not None:
        r = r + w_disc * r_disc.to(dtype)
    if r_enc is not None:
        r = r + w_enc * r_enc.to(dtype)
    advs = R.discount_values(dones.to(dtype), values.to(dtype), r, next_values.to(dtype), g32, gt32 / g32)
    return advs, advs + values.to(dtype)


def adv_norm(returns, values, mask, normalize, dtype=torch.float64):
    """learning/amp_agent.py:551-561 / learning/common_agent.py:536-546; returns, values [n, 1], mask [n] or None."""
    return R.calc_advs(returns.to(dtype), values.to(dtype), None if mask is None else mask.to(dtype), bool(normalize))


def adv_moments(returns, values, mask):
    """What phase 0 adds to acc3: sums over the f32 products (returns - values) * mask, accumulated in f64."""
    a = (returns.view(-1) - values.view(-1))
    m = torch.ones_like(a) if mask is None else mask.view(-1)
    am = (a * m).double()
    return torch.stack([m.double().sum(), am.sum(), (am * am).sum()])


def row_map(idx, remap, n):
    """include/ase_hip.h "row map": idx (or the row number), then env-major (env, t) -> time-major t*N + env."""
    p = torch.arange(n) if idx is None else idx[:n].long()
    if remap[0] > 0:
        H, N = remap
        p = (p % H) * N + p // H
    return p


def ring_store(src, D, idx, remap, n, dst, size, head):
    """learning/replay_buffer.py:27-49 on the mapped rows.  Returns the new ring."""
    out = dst.clone()
    out[(head + torch.arange(n)) % size] = src[row_map(idx, remap, n), :D]
    return out


# ------------------------------------------------------------------------------------------------ the rule
def allowance(ref32, ref64):
    d = (ref32.double() - ref64).abs()
    return 2 * float(d[torch.isfinite(d)].max() if torch.isfinite(d).any() else 0.0) + 1e-7


def within(got, ref64, ref32, name):
    """max |got - f64| <= 2 e_ref + 1e-7 over the finite entries; NaN / inf entries are equal as such.  Prints both numbers."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), (name, 'NaN entries differ')
    assert torch.equal(torch.isnan(ref32), torch.isnan(ref64)), (name, 'the reference disagrees with itself on NaN')
    fin = torch.isfinite(ref64)
    assert torch.equal(got[~fin & ~torch.isnan(ref64)], ref64[~fin & ~torch.isnan(ref64)]), (name, 'infinite entries differ')
    err = float((got[fin] - ref64[fin]).abs().max()) if fin.any() else 0.0
    tol = allowance(ref32, ref64)
    print(f'{name}: max |got - f64| = {err:.3g}, e_ref = {(tol - 1e-7) / 2:.3g}, allowance {tol:.3g}')
    assert err <= tol, (name, err, tol)
    return err, (tol - 1e-7) / 2


# ------------------------------------------------------------------------------------------------ input cases
NAN = float('nan')
SENTINEL = -1234.25


def disc_cases():
    """n in {1, 257}, ld > 1.  257: a sweep of [-30, 30], points on both sides of the clamp 1 - prob = 1e-4 (l = ln 9999 =
    9.21024), +-100, +-inf and NaN.  The other columns hold NaN: a kernel that reads them shows."""
    special = torch.tensor([9.2, 9.21, 9.2102, 9.21024, 9.2103, 9.2104, 9.22, 9.3, 100.0, -100.0, float('inf'), -float('inf'), NAN])
    sweep = torch.linspace(-30, 30, 257 - special.numel())
    out = []
    for name, col, ld, scale in (('n257', torch.cat([sweep, special]), 3, 2.0), ('n1', torch.tensor([0.3]), 2, 0.5)):
        logit = torch.full((col.numel(), ld), NAN)
        logit[:, 0] = col
        out.append({'name': name, 'logit': logit, 'n': col.numel(), 'scale': scale})
    return out


ROW_DIMS = (1, 64, 65, 128)


def row_cases():
    """enc_reward / normalize_rows operands: dim in ROW_DIMS, n = 11 (three blocks, the last ragged), ld > dim on both with NaN
    in the padding.  Row 2 all zero, row 3 all 1e-20 and row 6 all 1e-14 (the 1e-12 floor is active), row 4 z = -e / |e|
    (negative dot), row 5 NaN in its LAST column (the lane + 64 half when dim > 64)."""
    out = []
    for dim in ROW_DIMS:
        g = torch.Generator().manual_seed(100 + dim)
        n = 11
        e = torch.full((n, dim + 3), NAN)
        z = torch.full((n, dim + 5), NAN)
        e[:, :dim] = torch.randn(n, dim, generator=g) * 3
        zz = torch.randn(n, dim, generator=g)
        z[:, :dim] = zz / zz.norm(dim=-1, keepdim=True)
        e[2, :dim] = 0.0
        e[3, :dim] = 1e-20
        e[6, :dim] = 1e-14
        z[4, :dim] = -e[4, :dim] / e[4, :dim].norm()
        e[5, dim - 1] = NAN
        out.append({'name': f'dim{dim}', 'e': e, 'z': z, 'n': n, 'dim': dim, 'scale': 1.5, 'nan_rows': [5]})
    return out


GAE_SHAPES = ((1, 1), (1, 257), (32, 256), (7, 300))
DONES = ('none', 'all', 'last', 'random')


def gae_cases(H, N):
    """Every (r_disc, r_enc) presence x every dones pattern; a zero weight on the task term (all present) and on the
    discriminator term (no encoder)."""
    g = torch.Generator().manual_seed(1000 * H + N)
    out = []
    for has_d in (False, True):
        for has_e in (False, True):
            for dn in DONES:
                d = torch.zeros(H, N, dtype=torch.uint8)
                if dn == 'all':
                    d[:] = 1
                elif dn == 'last':
                    d[H - 1] = 1
                elif dn == 'random':
                    d = (torch.rand(H, N, generator=g) < 0.2).to(torch.uint8)
                t = [torch.randn(H, N, 1, generator=g) for _ in range(5)]
                w = (0.0, 0.5, 0.25) if (has_d and has_e) else ((0.7, 0.0, 0.0) if has_d else (0.3, 0.6, 0.9))
                out.append({'name': f'H{H} N{N} disc={int(has_d)} enc={int(has_e)} dones={dn}', 'dones': d, 'values': t[0],
                            'next_values': t[1], 'r_task': t[2], 'r_disc': t[3].abs() if has_d else None,
                            'r_enc': t[4].abs() if has_e else None, 'w': w, 'gamma': 0.99, 'tau': 0.95, 'H': H, 'N': N})
    return out


def adv_cases():
    """n in {2, 257, 9600} x masked / unmasked x normalize 0 / 1, and one pair with a common offset of 1e3 spreads in
    returns - values.  Every mask has at least two ones (asserted by the tests)."""
    out = []
    for n in (2, 257, 9600):
        for masked in (False, True):
            for offset in ((0.0, 100.0) if n == 9600 else (0.0,)):
                g = torch.Generator().manual_seed(n + 7 * masked)
                values = torch.randn(n, 1, generator=g)
                returns = values + offset + (0.1 if offset else 1.0) * torch.randn(n, 1, generator=g)
                mask = None
                if masked:
                    mask = (torch.rand(n, generator=g) < 0.7).float()
                    mask[:2] = 1.0
                for normalize in (0, 1):
                    out.append({'name': f'n{n} masked={int(masked)} normalize={normalize} offset={offset:g}', 'returns': returns,
                                'values': values, 'mask': mask, 'n': n, 'normalize': normalize})
    return out


RING_DIMS = (1, 64, 65, 140)


def ring_cases(D):
    """ld_src > D.  (a) no idx, no remap, full overwrite n == size from head = size - 1; (b) idx + remap, head + n wraps;
    (c) remap without idx; (d) idx without remap, no wrap, head 0."""
    g = torch.Generator().manual_seed(D)
    H, N = 5, 9                                            # 45 source rows
    src = torch.randn(H * N, D + 3, generator=g)
    out = []
    for name, use_idx, remap, n, size, head in (('a', False, (0, 0), 45, 45, 44), ('b', True, (H, N), 30, 37, 20),
                                                ('c', False, (H, N), 45, 50, 49), ('d', True, (0, 0), 13, 37, 0)):
        idx = torch.randperm(H * N, generator=g)[:n].to(torch.int32) if use_idx else None
        out.append({'name': f'D{D} {name}', 'src': src, 'D': D, 'idx': idx, 'remap': remap, 'n': n, 'size': size, 'head': head,
                    'ring': torch.randn(size, D, generator=g)})
    return out


# ------------------------------------------------------------------------------------------------ checks of a backend
# One body per operation, run on the emulator (CPU) by tests/test_rollout_ref.py and on the kernels by tests/test_gpu_rollout.py:
# b is the backend, dev its device.  Outputs are filled with SENTINEL first; what the call does not own must keep it.
def _d(t, dev):
    return None if t is None else t.to(dev)


def _filled(shape, dev, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype).to(dev)


def _kept(t):
    return bool((t == SENTINEL).all())


def check_disc_reward(b, dev, c, who):
    n, col = c['n'], c['logit'][:, 0]
    r = _filled((n + 2,), dev)
    b.disc_reward(_d(c['logit'], dev), r, n, c['scale'])
    ref64 = disc_reward(col, c['scale'])
    within(r[:n], ref64, disc_reward(col, c['scale'], torch.float32), f'{who} disc_reward {c["name"]}')
    assert _kept(r[n:])
    if n > 1:
        assert int(torch.isnan(ref64).sum()) == 1 and bool(torch.isnan(r.cpu()[:n][torch.isnan(col)]).all())
        assert abs(float(ref64[col == float('inf')]) - c['scale'] * 9.2103) < 1e-4 and float(ref64[col == -float('inf')]) == 0


def check_enc_reward(b, dev, c, who):
    n, dim = c['n'], c['dim']
    e, z = c['e'][:, :dim], c['z'][:, :dim]
    r = _filled((n + 1,), dev)
    b.enc_reward(_d(c['e'], dev), _d(c['z'], dev), r, n, dim, c['scale'])
    ref64 = enc_reward(e, z, c['scale'])
    within(r[:n], ref64, enc_reward(e, z, c['scale'], torch.float32), f'{who} enc_reward {c["name"]}')
    assert torch.isnan(ref64).nonzero().view(-1).tolist() == c['nan_rows']
    assert float(ref64[2]) == 0 and float(ref64[4]) == 0 and float(r[2]) == 0 and float(r[4]) == 0 and _kept(r[n:])


def check_normalize_rows(b, dev, c, who):
    n, dim = c['n'], c['dim']
    e = c['e'][:, :dim]
    y = _filled((n + 1, dim + 2), dev)
    b.normalize_rows(_d(c['e'], dev), y, n, dim)
    y64 = normalize_rows(e)
    within(y[:n, :dim], y64, normalize_rows(e, torch.float32), f'{who} normalize_rows {c["name"]}')
    assert bool(torch.isnan(y64[5]).all()) and not y64[2].any() and not y[2, :dim].any()
    assert _kept(y[n:]) and _kept(y[:, dim:])


def check_gae(b, dev, c, who):
    H, N = c['H'], c['N']
    advs, rets = _filled((H * N + 3,), dev), _filled((H * N + 3,), dev)
    args = (c['dones'], c['values'], c['next_values'], c['r_task'], c['r_disc'], c['r_enc'], *c['w'], c['gamma'], c['tau'])
    b.gae(*[_d(a, dev) if torch.is_tensor(a) else a for a in args], advs[:H * N].view(H, N, 1), rets[:H * N].view(H, N, 1), H, N)
    a64, r64 = gae(*args)
    a32, r32 = gae(*args, dtype=torch.float32)
    within(advs[:H * N], a64, a32, f'{who} gae advs {c["name"]}')
    within(rets[:H * N], r64, r32, f'{who} gae returns {c["name"]}')
    assert _kept(advs[H * N:]) and _kept(rets[H * N:])


def check_adv_norm(b, dev, c, who):
    n, mask, nz = c['n'], c['mask'], c['normalize']
    assert mask is None or float(mask.sum()) >= 2                      # a condition of the inputs: S - 1 > 0
    ret, val, m = _d(c['returns'], dev), _d(c['values'], dev), _d(mask, dev)
    acc3 = torch.zeros(3, dtype=torch.float64).to(dev)
    adv = _filled((n + 1,), dev)
    b.adv_norm(ret, val, m, adv, acc3, n, nz, 0)
    want = adv_moments(c['returns'], c['values'], mask)
    got = acc3.cpu()
    print(f'{who} adv_norm {c["name"]}: acc3 relative error {float(((got - want).abs() / want.abs()).max()):.3g}')
    assert bool(((got - want).abs() <= 1e-12 * want.abs()).all()), (got, want)
    assert _kept(adv)                                                  # phase 0 writes no advantage
    b.adv_norm(ret, val, m, adv, acc3, n, nz, 1)
    assert torch.equal(acc3.cpu(), got)                                # phase 1 only reads the sums
    within(adv[:n], adv_norm(c['returns'], c['values'], mask, nz), adv_norm(c['returns'], c['values'], mask, nz, torch.float32),
           f'{who} adv_norm {c["name"]}')
    if not nz:
        assert torch.equal(adv[:n].cpu(), (c['returns'] - c['values']).view(-1))
    assert _kept(adv[n:])


def check_ring_store(b, dev, c, who):
    ring = c['ring'].clone().to(dev)
    b.ring_store(_d(c['src'], dev), c['D'], _d(c['idx'], dev), c['remap'], c['n'], ring, c['size'], c['head'])
    want = ring_store(c['src'], c['D'], c['idx'], c['remap'], c['n'], c['ring'], c['size'], c['head'])
    assert torch.equal(ring.cpu(), want), c['name']
    written = torch.zeros(c['size'], dtype=torch.bool)
    written[(c['head'] + torch.arange(c['n'])) % c['size']] = True
    assert int(written.sum()) == c['n'] and torch.equal(want[~written], c['ring'][~written])
