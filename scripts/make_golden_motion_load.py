"""Golden vectors of the clip loader: the reference's OWN MotionLib (utils/motion_lib.py, poselib loader) on
the committed copies of shipped clip files under tests/golden/clips/ -

  a   three.yaml: three sword-and-shield clips (17 bodies, 31 dofs) with unequal weights
  b   amp_humanoid_run.npy: the 15-body skeleton with the 28-dof tables (env/tasks/humanoid.py:184-185)
  c   RL_Avatar_TurnLeft90_Motion.npy alone, with a joint table of its own that puts a 3-dof and a 1-dof joint on bodies whose
      stored rotation never changes (6, 9, 10: sword, shield, left hand) - the only frame pairs with angle == 0 in these
      clips; the tables of (a) and (b) have no joint there

For each: the six frame arrays the loader leaves (gts, grs, lrs, grvs, gravs, dvs), the per-clip tables, the normalised
weights, and get_motion_state at seeded (motion id, time) pairs chosen as oracle/make_golden_motion.py does (start, exact end,
past the end, exactly on a frame).  Quaternion primitives of get_motion_state: the isaacgym restatement of
oracle/rl_games_shim.  The first two clips of (a) are those of tests/golden/motion_state.pt; the script asserts that their
arrays reproduce that file bitwise.

    python scripts/make_golden_motion_load.py      # needs the reference tree; writes tests/golden/motion_load.pt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('ASE_REFERENCE', '/root/reference/ase')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'rl_games_shim'))
sys.path.insert(0, REFERENCE)

from utils.motion_lib import MotionLib        # noqa: E402  (reference code)

CLIP_DIR = os.path.join(ROOT, 'tests', 'golden', 'clips')
CASES = {
    'a': {'motion_file': 'three.yaml',
          'dof_body_ids': [1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 16],            # env/tasks/humanoid.py:191-192
          'dof_offsets': [0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 28, 31],
          'key_body_ids': [5, 10, 13, 16, 6, 9], 'seed': 78},
    'b': {'motion_file': 'amp_humanoid_run.npy',
          'dof_body_ids': [1, 2, 3, 4, 6, 7, 9, 10, 11, 12, 13, 14],                # env/tasks/humanoid.py:184-185
          'dof_offsets': [0, 3, 6, 9, 10, 13, 14, 17, 18, 21, 24, 25, 28],
          'key_body_ids': [5, 8, 11, 14], 'seed': 79},                               # right_hand, left_hand, right_foot, left_foot
    'c': {'motion_file': 'RL_Avatar_TurnLeft90_Motion.npy', 'dof_body_ids': [1, 6, 4, 9, 10, 14],
          'dof_offsets': [0, 3, 6, 7, 8, 11, 14], 'key_body_ids': [6, 16], 'seed': 80},
}
OUT_NAMES = ('root_pos', 'root_rot', 'dof_pos', 'root_vel', 'root_ang_vel', 'dof_vel', 'key_pos')


def record(case):
    ml = MotionLib(motion_file=os.path.join(CLIP_DIR, case['motion_file']), dof_body_ids=case['dof_body_ids'],
                   dof_offsets=case['dof_offsets'], key_body_ids=case['key_body_ids'], device='cpu')
    g = torch.Generator().manual_seed(case['seed'])
    n = 200
    ids = torch.randint(0, ml.num_motions(), (n,), generator=g)
    lens = ml._motion_lengths[ids]
    t = torch.rand(n, generator=g) * lens
    t[0], t[1], t[2] = 0.0, lens[1], lens[2] + 0.5                       # start, exact end, past the end (clipped phase)
    t[3] = ml._motion_dt[ids[3]] * 7                                     # exactly on a frame
    out = ml.get_motion_state(ids, t)
    return {'motion_file': case['motion_file'], 'dof_body_ids': case['dof_body_ids'], 'dof_offsets': case['dof_offsets'],
            'key_body_ids': case['key_body_ids'],
            'motion_files': [os.path.basename(f) for f in ml._motion_files],
            'clips': {'gts': ml.gts, 'grs': ml.grs, 'lrs': ml.lrs, 'grvs': ml.grvs, 'gravs': ml.gravs, 'dvs': ml.dvs,
                      'lengths': ml._motion_lengths, 'num_frames': ml._motion_num_frames, 'dt': ml._motion_dt,
                      'length_starts': ml.length_starts},
            'weights': ml._motion_weights, 'fps': ml._motion_fps, 'motion_ids': ids, 'times': t,
            'outputs': {k: v.clone() for k, v in zip(OUT_NAMES, out)}}


def main():
    G = {name: record(case) for name, case in CASES.items()}
    # (a)'s first two clips are the clips of motion_state.pt: same files, same loader, so the same bits
    M = torch.load(os.path.join(ROOT, 'tests', 'golden', 'motion_state.pt'), weights_only=False)['clips']
    T2 = M['gts'].shape[0]
    for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs'):
        assert torch.equal(G['a']['clips'][k][:T2], M[k]), f'clip array {k} differs from tests/golden/motion_state.pt'
    for k in ('lengths', 'num_frames', 'dt', 'length_starts'):
        assert torch.equal(G['a']['clips'][k][:2], M[k]), k
    for name in CASES:
        for k, v in G[name]['clips'].items():
            assert v.dtype in (torch.float32, torch.int64), (k, v.dtype)
    path = os.path.join(ROOT, 'tests', 'golden', 'motion_load.pt')
    torch.save(G, path)
    print('wrote', path, {n: tuple(G[n]['clips']['gts'].shape) for n in G}, '%.1f KB' % (os.path.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
