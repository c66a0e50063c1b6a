"""EmuBackend with the learned action log-std (rl_games learn_sigma): the keyword arguments ls_mode / d_logstd / db_logstd /
entropy_coef of ppo_head, the per-row log-std of sample_actions and the bias-only Adam-table row of the learned vector.
Test infrastructure, the CPU counterpart of csrc/heads.hip LS_VECTOR / LS_ROWS and csrc/rollout.hip's ld_logstd."""
import math

import torch

from ase_amd import lib as L
from tests.emu_backend import EmuBackend, _dyn, _report, _store


class LearnedSigmaEmu(EmuBackend):
    def ppo_head(self, mu, value, mb, new_z, logstd, d_mu, d_value, db_mu, db_value, acc, M, m_global, act_dim,
                 z_dim, masked, div_on, mu_tanh, clip_value, e_clip, critic_coef, bounds_coef, div_coef, div_tar,
                 mu_out=None, grad_scale=1.0, dyn=None, ls_mode=L.LS_FROZEN, d_logstd=None, db_logstd=None, entropy_coef=0.0):
        if ls_mode == L.LS_FROZEN:
            return super().ppo_head(mu, value, mb, new_z, logstd, d_mu, d_value, db_mu, db_value, acc, M, m_global, act_dim,
                                    z_dim, masked, div_on, mu_tanh, clip_value, e_clip, critic_coef, bounds_coef, div_coef,
                                    div_tar, mu_out=mu_out, grad_scale=grad_scale, dyn=dyn)
        D, gs = act_dim, float(grad_scale) * _dyn(dyn)
        # the frozen head's arithmetic on a zero log-std vector, then the terms a learned log-std changes are redone below
        ls = (logstd[:M, :D] if ls_mode == L.LS_ROWS else logstd[:D].expand(M, D)).float()
        raw = mu[:M, :D]
        m = torch.tanh(raw) if mu_tanh else raw
        a, omu, osg = mb['actions'], mb['mu'], mb['sigma']
        sg = torch.exp(ls)
        d = (a - m) / sg
        nlp = 0.5 * (d * d).sum(-1) + 0.5 * math.log(2 * math.pi) * D + ls.sum(-1)
        ratio = torch.exp(mb['old_logp_actions'].view(-1) - nlp)
        adv = mb['advantages'].view(-1)
        rc = torch.clamp(ratio, 1 - e_clip, 1 + e_clip)
        s1, s2 = -adv * ratio, -adv * rc
        a_loss = torch.max(s1, s2)
        g = torch.where(ratio == rc, -adv, torch.where(s1 > s2, -adv, torch.where(s1 == s2, -0.5 * adv, torch.zeros_like(adv))))
        S = float(acc[L.ACC_MASK_SUM]) if masked else float(m_global)
        mk = mb['rand_action_mask'].view(-1) if masked else torch.ones(M)
        w = mk / S
        bh, bl = torch.clamp_min(m - 1, 0), torch.clamp_max(m + 1, 0)
        b_row = (bh * bh + bl * bl).sum(-1)
        ent_row = (0.5 + 0.5 * math.log(2 * math.pi) + ls).sum(-1)
        kl_row = (torch.log(osg / sg + 1e-5) + (sg * sg + (omu - m) ** 2) / (2 * (osg * osg + 1e-5)) - 0.5).sum(-1)
        gm = (w * g * ratio).unsqueeze(-1) * d / sg + bounds_coef * w.unsqueeze(-1) * 2 * (bh + bl)
        gl = w.unsqueeze(-1) * (-(g * ratio).unsqueeze(-1) * (1 - d * d) - entropy_coef)
        div_row = torch.zeros(M)
        gm2 = None
        if div_on:
            raw2 = mu[M:2 * M, :D]
            m2 = torch.tanh(raw2) if mu_tanh else raw2
            cm, cm2 = torch.clamp(m, -1, 1), torch.clamp(m2, -1, 1)
            diff = cm - cm2
            a_diff = (diff * diff).sum(-1) / D
            zz = (new_z[:M] * mb['ase_latents']).sum(-1)
            inv = 1.0 / (0.5 - 0.5 * zz + 1e-5)
            bonus = a_diff * inv
            div_row = (div_tar - bonus) ** 2
            dl = div_coef * w * 2 * (bonus - div_tar)
            db = (dl * inv).unsqueeze(-1) * 2 * diff / D
            gm = gm + db * ((m >= -1) & (m <= 1))
            gm2 = -db * ((m2 >= -1) & (m2 <= 1))
            if mu_tanh:
                gm2 = gm2 * (1 - m2 * m2)
        if mu_tanh:
            gm = gm * (1 - m * m)
        o1 = _store(gs * gm, d_mu.dtype)
        d_mu[:M, :D] = o1
        dbm = o1.float().sum(0) / gs
        if div_on:
            o2 = _store(gs * gm2, d_mu.dtype)
            d_mu[M:2 * M, :D] = o2
            dbm = dbm + o2.float().sum(0) / gs
        ol = _store(gs * gl, d_mu.dtype)
        if d_logstd is not None:
            d_logstd[:M, :D] = ol
            if div_on:
                d_logstd[M:2 * M, :D] = 0
        v = value[:M, 0]
        R = mb['returns'].view(-1)
        if clip_value:
            ov = mb['old_values'].view(-1)
            dlt = v - ov
            vpc = ov + torch.clamp(dlt, -e_clip, e_clip)
            l1, l2 = (v - R) ** 2, (vpc - R) ** 2
            c = torch.max(l1, l2)
            g1, g2 = 2 * (v - R), 2 * (vpc - R) * ((dlt >= -e_clip) & (dlt <= e_clip))
            dv = torch.where(l1 > l2, g1, torch.where(l1 < l2, g2, 0.5 * (g1 + g2)))
        else:
            c = (R - v) ** 2
            dv = 2 * (v - R)
        ov_ = _store(gs * (critic_coef * dv / m_global), d_value.dtype)
        d_value[:M, 0] = ov_
        _report(dyn, ov_, d_mu[:2 * M if div_on else M, :D], ol)
        if db_mu is not None:
            db_mu[:D] += dbm
            if db_value is not None:
                db_value[0] += ov_.float().sum() / gs
        if db_logstd is not None:
            db_logstd[:D] += ol.float().sum(0) / gs
        if mu_out is not None:
            mu_out[:M, :D] = m
        acc[L.ACC_A_LOSS] += (mk * a_loss).double().sum()
        acc[L.ACC_B_LOSS] += (mk * b_row).double().sum()
        acc[L.ACC_ENTROPY] += (mk * ent_row).double().sum()
        acc[L.ACC_CLIPPED] += (mk * ((ratio - 1).abs() > e_clip)).double().sum()
        acc[L.ACC_C_LOSS] += c.double().sum()
        acc[L.ACC_KL] += kl_row.double().sum()
        if div_on:
            acc[L.ACC_DIV] += (mk * div_row).double().sum()

    def sample_actions(self, mu, logstd, rand_probs, rng_state, mu_out, sigma_out, actions, neglogp, rand_mask, n, act_dim,
                       mu_tanh=False, logstd_rows=False):
        if not logstd_rows:
            return super().sample_actions(mu, logstd, rand_probs, rng_state, mu_out, sigma_out, actions, neglogp, rand_mask, n,
                                          act_dim, mu_tanh)
        g = torch.Generator().manual_seed(int(rng_state[0]) * 1000003 + int(rng_state[1]) + 17)
        m = mu[:n, :act_dim].float()
        if mu_tanh:
            m = torch.tanh(m)
        ls = logstd[:n, :act_dim].float()
        s = torch.exp(ls)
        a = m + s * torch.randn(n, act_dim, generator=g)
        nlp = 0.5 * (((a - m) / s) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * act_dim + ls.sum(-1)
        keep = torch.ones(n)
        if rand_probs is not None:
            keep = torch.bernoulli(rand_probs[:n].float().cpu(), generator=g)
        mu_out[:n] = m
        sigma_out[:n] = s
        actions[:n] = torch.where(keep.view(-1, 1) != 0, a, m)
        neglogp.view(-1)[:n] = nlp
        if rand_mask is not None:
            rand_mask.view(-1)[:n] = keep
        rng_state[1] += 1

    def apply_multi(self, desc, items, dtype, opt_state, acc):
        # bias-only rows (the learned log-std vector: no weight matrix, no shadows) take Adam on the vector alone
        rest = []
        for it in items:
            if it[0].numel() == 0:
                b, bs, gb, mb, vb = it[5], it[6], it[10], it[11], it[12]
                if opt_state is not None:
                    self.adam(b, gb, mb, vb, opt_state)
                bs[:b.numel()] = b
            else:
                rest.append(it)
        if rest:
            super().apply_multi(desc, rest, dtype, opt_state, acc)
