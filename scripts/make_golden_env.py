"""Golden vectors of the environment-side tensor functions, recorded from the reference's own jit functions:
compute_humanoid_observations_max and compute_humanoid_reset (env/tasks/humanoid.py), the strike form of the reset and the
observation / reward functions of humanoid_heading, humanoid_location, humanoid_reach and humanoid_strike, imported unmodified
and run on the CPU in f32 and - on the same inputs cast up - in f64.  TEST INFRASTRUCTURE ONLY (needs the reference tree; its
quaternion primitives come from the isaacgym restatement in oracle/rl_games_shim, as for tests/golden/amp_obs.pt).

    python scripts/make_golden_env.py            # writes tests/golden/env_tensors.pt (tensors and plain lists only)

What the file carries and why:
  inputs            seeded state of N = 96 environments x 17 bodies; rows 0-3 take the edge branches (identity root rotation,
                    half turn about z, x axis straight down = heading from atan2(0, 0), target at the root's own xy position)
  f32 / f64         every function's output in both precisions.  The four flag combinations of the humanoid observation
                    differ only in column 0 and the root's six rotation columns (asserted here, bitwise): the file keeps the
                    full matrix of (local_root_obs, root_height_obs) = (True, True) and those seven columns of the others
  e_ref             per function max |f32 - f64| of the REFERENCE, the larger of the fixture's rows and a seeded 4096-row
                    draw from the same distribution: the allowance of the device tests (2 e_ref + 1e-7 against f64)
  margins           the rewards and resets branch on float thresholds.  A row whose decision quantity lies within 1e-3 of
                    its threshold is re-drawn, so two correct f32 implementations cannot disagree on a branch; the f32 and
                    the f64 run agree on every mask, and every branch is taken by >= 4 rows and not taken by >= 4 (asserted).
                    Row 3 is exempt for the location / strike speed mask: normalize(0) = 0 makes its speed exactly 0.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('ASE_REFERENCE', '/root/reference/ase')
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'rl_games_shim'))
sys.path.insert(0, REFERENCE)

from env.tasks import humanoid as H                # noqa: E402  (reference code)
from env.tasks import humanoid_heading as HH       # noqa: E402
from env.tasks import humanoid_location as HL      # noqa: E402
from env.tasks import humanoid_reach as HR         # noqa: E402
from env.tasks import humanoid_strike as HS        # noqa: E402

N, B = 96, 17
MARGIN, E_REF_MAX = 1e-3, 2e-5
# sword & shield humanoid: feet may touch the ground; the strike task's sword / shield arm bodies may touch the target
CONTACT_BODY_IDS = [11, 14]
STRIKE_BODY_IDS = [4, 5, 6, 8, 9, 10]
REACH_BODY_ID = 5
MAX_EPISODE_LENGTH = 300.0
DT = 1.0 / 30.0
TAR_SPEED = 1.0          # humanoid_location's scalar target speed
ENV_IDS = [5, 0, 17, 2, 95, 3, 40, 41, 42, 64, 1]
SPECIAL = 4              # rows 0-3 are set by hand


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def draw(n, g, special):
    """One seeded state.  Unit scale throughout (positions in metres, a step of 1/30 s)."""
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    rot = unit(r(n, B, 4))
    root_pos = r(n, 3) * torch.tensor([3.0, 3.0, 0.3]) + torch.tensor([0.0, 0.0, 0.9])
    pos = root_pos.unsqueeze(1) + r(n, B, 3) * torch.tensor([0.5, 0.5, 0.35])
    pos[:, 0] = root_pos
    vel, ang = r(n, B, 3) * 2, r(n, B, 3) * 3
    I = {'body_pos': pos, 'body_rot': rot, 'body_vel': vel, 'body_ang_vel': ang}
    I['prev_root_pos'] = root_pos - r(n, 3) * 1.5 * DT
    I['tar_dir'] = unit(r(n, 2))
    I['tar_face_dir'] = unit(r(n, 2))
    I['tar_speed'] = 1.0 + 4.0 * u(n)
    I['tar_pos_loc'] = root_pos[:, :2] + r(n, 2) * 0.8
    I['tar_pos_reach'] = pos[:, REACH_BODY_ID] + r(n, 3) * 0.4
    tar_pos = root_pos + r(n, 3) * torch.tensor([2.0, 2.0, 0.3])
    I['tar_states'] = torch.cat([tar_pos, unit(r(n, 4)), r(n, 3), r(n, 3) * 2], -1)
    # contact forces: quiet everywhere (|f| <= 0.05), loud on some bodies of half of the rows, always loud on the feet
    contact = (u(n, B, 3) - 0.5) * 0.1
    loud = (u(n, 1, 1) < 0.5) & (u(n, B, 1) < 0.2)
    contact = torch.where(loud, r(n, B, 3) * 3, contact)
    contact[:, CONTACT_BODY_IDS] = r(n, len(CONTACT_BODY_IDS), 3) * 5
    I['contact_forces'] = contact
    I['tar_contact_forces'] = r(n, 3) * 2
    heights = torch.full((B,), 0.15)
    heights[[3, 7]] = 0.3
    I['termination_heights'] = heights
    progress = torch.randint(0, int(MAX_EPISODE_LENGTH), (n,), generator=g)
    if special:
        m = int(MAX_EPISODE_LENGTH)
        edge = torch.tensor([0, 1, 2, m - 2, m - 1] * 5)              # integer thresholds: both sides, on purpose
        progress[SPECIAL:SPECIAL + edge.numel()] = edge
        set_special(I)
    I['progress_buf'] = progress
    return I


def set_special(I):
    q = I['body_rot']
    q[0, 0] = torch.tensor([0.0, 0.0, 0.0, 1.0])                                   # identity
    q[1, 0] = torch.tensor([0.0, 0.0, 1.0, 0.0])                                   # half turn about z (heading = pi)
    q[2, 0] = torch.tensor([0.0, 0.7071067811865476, 0.0, 0.7071067811865476])     # x axis points down: heading from (0, 0)
    I['tar_pos_loc'][3] = I['body_pos'][3, 0, :2]                                  # target at the root's own xy position
    I['tar_states'][3, :2] = I['body_pos'][3, 0, :2]


def root_states(I):
    return torch.cat([I['body_pos'][:, 0], I['body_rot'][:, 0], I['body_vel'][:, 0], I['body_ang_vel'][:, 0]], -1).contiguous()


def cast(I, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in I.items()}


def run(I, dtype):
    """Every function of the reference on one precision."""
    I = cast(I, dtype)
    rs = root_states(I)
    root_pos, root_rot = rs[:, 0:3].contiguous(), rs[:, 3:7].contiguous()
    O = {}
    for lr in (True, False):
        for rh in (True, False):
            O[('obs_max', lr, rh)] = H.compute_humanoid_observations_max(I['body_pos'], I['body_rot'], I['body_vel'],
                                                                         I['body_ang_vel'], lr, rh)
    O['heading_obs'] = HH.compute_heading_observations(rs, I['tar_dir'], I['tar_speed'], I['tar_face_dir'])
    O['heading_rew'] = HH.compute_heading_reward(root_pos, I['prev_root_pos'], root_rot, I['tar_dir'], I['tar_speed'],
                                                 I['tar_face_dir'], DT)
    O['location_obs'] = HL.compute_location_observations(rs, I['tar_pos_loc'])
    O['location_rew'] = HL.compute_location_reward(root_pos, I['prev_root_pos'], root_rot, I['tar_pos_loc'], TAR_SPEED, DT)
    O['reach_obs'] = HR.compute_location_observations(rs, I['tar_pos_reach'])
    O['reach_rew'] = HR.compute_reach_reward(I['body_pos'][:, REACH_BODY_ID].contiguous(), root_rot, I['tar_pos_reach'], TAR_SPEED, DT)
    ts = I['tar_states']
    O['strike_obs'] = HS.compute_strike_observations(rs, ts)
    O['strike_rew'] = HS.compute_strike_reward(ts[:, 0:3].contiguous(), ts[:, 3:7].contiguous(), rs, I['prev_root_pos'],
                                               I['body_vel'][:, STRIKE_BODY_IDS[0]].contiguous(), DT, 1.4)
    n = rs.shape[0]
    reset_buf = torch.ones(n, dtype=torch.long)
    cb, sb = torch.tensor(CONTACT_BODY_IDS), torch.tensor(STRIKE_BODY_IDS)
    for early in (True, False):
        O[('reset', 'plain', early)] = H.compute_humanoid_reset(reset_buf, I['progress_buf'], I['contact_forces'], cb, I['body_pos'],
                                                                MAX_EPISODE_LENGTH, early, I['termination_heights'])
        O[('reset', 'strike', early)] = HS.compute_humanoid_reset(reset_buf, I['progress_buf'], I['contact_forces'], cb, I['body_pos'],
                                                                  I['tar_contact_forces'], sb, MAX_EPISODE_LENGTH, early,
                                                                  I['termination_heights'])
    return O


def decisions(I, dtype):
    """name -> (quantity [n, k], threshold [k] or scalar): the float quantities the reference compares with a threshold,
    computed the way it computes them (reference lines in ase_amd/csrc/env_obs.hip)."""
    I = cast(I, dtype)
    root = I['body_pos'][:, 0]
    root_vel = (root - I['prev_root_pos']) / DT
    D = {}
    D['heading_speed'] = ((I['tar_dir'] * root_vel[:, :2]).sum(-1, keepdim=True), 0.0)
    diff = I['tar_pos_loc'] - root[:, :2]
    D['location_pos_err'] = ((diff * diff).sum(-1, keepdim=True), 0.5)
    D['location_speed'] = ((torch.nn.functional.normalize(diff, dim=-1) * root_vel[:, :2]).sum(-1, keepdim=True), 0.0)
    sdir = torch.nn.functional.normalize(I['tar_states'][:, :2] - root[:, :2], dim=-1)
    D['strike_speed'] = ((sdir * root_vel[:, :2]).sum(-1, keepdim=True), 0.0)
    q = I['tar_states'][:, 3:7]
    D['strike_rot_err'] = ((2.0 * q[:, 3:4] ** 2 - 1.0) + 2.0 * q[:, 2:3] * q[:, 2:3], 0.2)       # z of the rotated z axis
    c = I['contact_forces'].abs().reshape(root.shape[0], -1)
    D['contact_0.1'] = (c, 0.1)
    D['contact_1.0'] = (c, 1.0)
    D['height'] = (I['body_pos'][..., 2], I['termination_heights'])
    D['tar_contact'] = (I['tar_contact_forces'][:, :2].abs(), 1.0)
    return D


EXEMPT = {'location_speed': [3], 'strike_speed': [3]}      # exactly 0 by construction (normalize of a zero vector)


def near_threshold(I, special):
    bad = torch.zeros(I['body_pos'].shape[0], dtype=torch.bool)
    for name, (qty, thr) in decisions(I, torch.float64).items():
        near = ((qty - thr).abs() < MARGIN).any(-1)
        if special:
            near[EXEMPT.get(name, [])] = False
        bad |= near
    return bad


def draw_with_margins(n, g, special):
    I = draw(n, g, special)
    for _ in range(50):
        bad = near_threshold(I, special)
        if not bad.any():
            break
        J = draw(n, g, False)
        for k, v in I.items():
            if v.dim() > 0 and v.shape[0] == n and k != 'progress_buf':
                v[bad] = J[k][bad]
        if special:
            set_special(I)
    assert not near_threshold(I, special).any(), 'a decision quantity is still within the margin of its threshold'
    return I


def masks(I, O, dtype):
    """Every boolean the reference branches on, per row."""
    D = decisions(I, dtype)
    M = {'heading_speed<=0': D['heading_speed'][0][:, 0] <= 0, 'location_speed<=0': D['location_speed'][0][:, 0] <= 0,
         'location_pos_err<0.5': D['location_pos_err'][0][:, 0] < 0.5, 'strike_speed<=0': D['strike_speed'][0][:, 0] <= 0,
         'strike_rot_err<0.2': D['strike_rot_err'][0][:, 0] < 0.2}
    I = cast(I, dtype)
    keep = torch.ones(B, dtype=torch.bool)
    keep[CONTACT_BODY_IDS] = False
    nonstrike = keep.clone()
    nonstrike[STRIKE_BODY_IDS] = False
    c = I['contact_forces'].abs().amax(-1)
    M['fall_contact'] = (c[:, keep] > 0.1).any(-1)
    M['fall_height'] = (I['body_pos'][..., 2] < I['termination_heights'])[:, keep].any(-1)
    M['has_fallen'] = M['fall_contact'] & M['fall_height']
    M['tar_has_contact'] = (I['tar_contact_forces'][:, :2].abs() > 1.0).any(-1)
    M['nonstrike_contact'] = (c[:, nonstrike] > 1.0).any(-1)
    M['tar_fail'] = M['tar_has_contact'] & M['nonstrike_contact']
    M['progress>1'] = I['progress_buf'] > 1
    M['progress>=max-1'] = I['progress_buf'] >= MAX_EPISODE_LENGTH - 1
    for form in ('plain', 'strike'):
        M[f'terminated_{form}'] = O[('reset', form, True)][1] > 0
        M[f'reset_{form}'] = O[('reset', form, True)][0] > 0
    return M


FLOAT_FUNCS = ['obs_max', 'heading_obs', 'heading_rew', 'location_obs', 'location_rew', 'reach_obs', 'reach_rew', 'strike_obs',
               'strike_rew']


def ref_error(O32, O64):
    e = {}
    for name in FLOAT_FUNCS:
        keys = [k for k in O32 if k == name or (isinstance(k, tuple) and k[0] == name)]
        e[name] = max(float((O32[k].double() - O64[k]).abs().max()) for k in keys)
    return e


def build():
    g = torch.Generator().manual_seed(20261)
    I = draw_with_margins(N, g, True)
    O32, O64 = run(I, torch.float32), run(I, torch.float64)
    M32, M64 = masks(I, O32, torch.float32), masks(I, O64, torch.float64)
    counts = {}
    for k in M32:
        assert torch.equal(M32[k], M64[k]), f'the f32 and the f64 run disagree on {k}'
        counts[k] = [int(M32[k].sum()), int((~M32[k]).sum())]
        assert min(counts[k]) >= 4, f'branch {k} taken by {counts[k][0]} rows, not taken by {counts[k][1]}'
    for k in O32:
        if k[0] == 'reset':
            assert all(torch.equal(a, b) for a, b in zip(O32[k], O64[k])), k
    # edge rows hit the integer thresholds on both sides with a fall pending
    assert {0, 1, 2, 298, 299} <= set(I['progress_buf'].tolist())
    # the allowance: what the reference's own f32 run loses against f64, here and on a larger draw of the same distribution
    e_fix = ref_error(O32, O64)
    big = draw_with_margins(4096, torch.Generator().manual_seed(20262), False)
    e_big = ref_error(run(big, torch.float32), run(big, torch.float64))
    e_ref = {k: max(e_fix[k], e_big[k]) for k in FLOAT_FUNCS}
    for k, v in e_ref.items():
        assert v <= E_REF_MAX, f'{k}: the reference itself loses {v:.3g} in f32 - an ill-conditioned row'
    # compact form of the four flag combinations of the humanoid observation
    o_rot = 1 + 3 * (B - 1)
    cols = [0] + list(range(o_rot, o_rot + 6))
    rest = [c for c in range(15 * B - 2) if c not in cols]
    G = {'num_envs': N, 'num_bodies': B, 'contact_body_ids': CONTACT_BODY_IDS, 'strike_body_ids': STRIKE_BODY_IDS,
         'reach_body_id': REACH_BODY_ID, 'max_episode_length': MAX_EPISODE_LENGTH, 'dt': DT, 'tar_speed': TAR_SPEED,
         'env_ids': ENV_IDS, 'margin': MARGIN, 'exempt': {k: list(v) for k, v in EXEMPT.items()}, 'obs_max_flag_cols': cols,
         'inputs': {k: v.clone() for k, v in I.items()}, 'e_ref': e_ref, 'e_ref_fixture': e_fix, 'e_ref_4096': e_big,
         'branch_counts': counts}
    G['inputs']['root_states'] = root_states(I)
    for tag, O in (('f32', O32), ('f64', O64)):
        out = {}
        base = O[('obs_max', True, True)]
        out['obs_max'] = base.clone()
        out['obs_max_flag_cols'] = {}
        for lr in (True, False):
            for rh in (True, False):
                o = O[('obs_max', lr, rh)]
                assert torch.equal(o[:, rest], base[:, rest]), 'flag combinations differ outside the seven columns'
                out['obs_max_flag_cols'][(lr, rh)] = o[:, cols].clone()
        for k in FLOAT_FUNCS[1:]:
            out[k] = O[k].clone()
        for form in ('plain', 'strike'):
            for early in (True, False):
                r, t = O[('reset', form, early)]
                out[('reset', form, early)] = (r.clone(), t.clone())
        G[tag] = out
    # the subset call of the reference: its function on the gathered rows (env/tasks/humanoid.py:399-413)
    ids = torch.tensor(ENV_IDS)
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        J = cast(I, dt)
        G[tag]['obs_max_subset'] = H.compute_humanoid_observations_max(J['body_pos'][ids], J['body_rot'][ids], J['body_vel'][ids],
                                                                       J['body_ang_vel'][ids], True, True).clone()
        assert torch.equal(G[tag]['obs_max_subset'], G[tag]['obs_max'][ids])
    return G


def main():
    G = build()
    path = os.path.join(ROOT, 'tests', 'golden', 'env_tensors.pt')
    torch.save(G, path)
    print('wrote', path, os.path.getsize(path), 'bytes')
    for k in FLOAT_FUNCS:
        print(f'  e_ref {k:13s} fixture {G["e_ref_fixture"][k]:.3g}  4096 rows {G["e_ref_4096"][k]:.3g}')
    print('  branch counts', G['branch_counts'])


if __name__ == '__main__':
    main()
