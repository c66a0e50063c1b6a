"""Golden vectors of the retargeter: the reference's OWN poselib - ``SkeletonMotion.retarget_to_by_tpose``, the
trim, ``project_joints`` of poselib/retarget_motion.py, the grounding and ``SkeletonMotion.from_skeleton_state``, i.e. the calls
of ``retarget_motion.main()`` without its file paths and plots - on seeded synthetic source motions: a per-joint sinusoidal
axis-angle on the T-pose plus a moving root (the reference's own .fbx sources need the FBX SDK).

  cmu        38 -> 15 bodies, T-pose stored in global form, the shipped config; clips of 2, 18 and 40 frames at 120, 60, 30 fps,
             the 40-frame clip trimmed to [5, 33)
  sfu        30 -> 15 bodies, local T-pose, its shipped config; clips of 3 and 17 frames
  global     the cmu 18-frame clip re-saved by poselib with is_local == False
  unmapped   target: the 17-body tree of tests/golden/clips/RL_Avatar_TurnLeft90_Motion.npy in zero pose, the 15 common names
             mapped - sword and shield inherit an ancestor
  nohinge    cmu without project_joints
  topology   as unmapped with LeftHand -> shield and LeftFingerBase -> left_hand: the reduced target tree hangs both under
             left_lower_arm while the source chains them, so recomposing along the wrong reduced tree shows

For each case: the inputs (source clips as f32 arrays), per clip the reference's result after each stage, and the names of the
T-pose / config files under tests/golden/retarget/ (byte copies of the reference's data files, made here).

    python scripts/make_golden_retarget.py [--time]     # needs the reference tree; CPU only
"""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('ASE_REFERENCE', '/root/reference/ase')
POSELIB = os.path.join(REFERENCE, 'poselib')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'rl_games_shim'))
sys.path.insert(0, POSELIB)

import retarget_motion as RM                                                       # noqa: E402  (reference code)
from poselib.core.rotation3d import quat_from_angle_axis, quat_mul_norm           # noqa: E402
from poselib.skeleton.skeleton3d import SkeletonMotion, SkeletonState             # noqa: E402

OUT_DIR = os.path.join(ROOT, 'tests', 'golden', 'retarget')
CLIP_DIR = os.path.join(ROOT, 'tests', 'golden', 'clips')
DATA_FILES = ('cmu_tpose.npy', 'sfu_tpose.npy', 'amp_humanoid_tpose.npy')
CONFIGS = ('retarget_cmu_to_amp.json', 'retarget_sfu_to_amp.json')


def synthesize(tpose, frames, fps, seed, scale):
    """A smooth motion on the T-pose's skeleton: local rotation = T-pose local * exp(a_j sin(w_j t + p_j)), amplitudes near
    0.5 rad; the root walks and bobs (in the skeleton's own units: 1 / scale)."""
    g = torch.Generator().manual_seed(seed)
    B = len(tpose.skeleton_tree)
    axis = torch.randn(B, 3, generator=g)
    amp = 0.35 + 0.3 * torch.rand(B, generator=g)
    freq = 2.0 + 6.0 * torch.rand(B, generator=g)
    phase = 6.283 * torch.rand(B, generator=g)
    t = torch.arange(frames, dtype=torch.float32) / fps
    angle = amp * torch.sin(freq * t[:, None] + phase)                                             # [F, B]
    rot = quat_mul_norm(tpose.local_rotation.unsqueeze(0), quat_from_angle_axis(angle, axis.unsqueeze(0).expand(frames, B, 3)))
    unit = 1.0 / scale
    root = tpose.root_translation.unsqueeze(0) + unit * torch.stack(
        [1.2 * t, 0.3 * torch.sin(2.0 * t + float(phase[0])), 0.05 * torch.sin(5.0 * t)], dim=-1)
    state = SkeletonState.from_rotation_and_root_translation(tpose.skeleton_tree, rot.float(), root.float(), is_local=True)
    return SkeletonMotion.from_skeleton_state(state, fps=fps)


def run_reference(source_motion, source_tpose, target_tpose, cfg, trim, hinges=True):
    """retarget_motion.main() from `source_motion.retarget_to_by_tpose` on, without files and plots."""
    target_motion = source_motion.retarget_to_by_tpose(
        joint_mapping=cfg['joint_mapping'], source_tpose=source_tpose, target_tpose=target_tpose,
        rotation_to_target_skeleton=torch.tensor(cfg['rotation']), scale_to_target_skeleton=cfg['scale'])
    out = {'pose_rotation': target_motion.local_rotation.clone(), 'pose_root': target_motion.root_translation.clone()}
    frame_beg, frame_end = trim
    if frame_beg == -1:
        frame_beg = 0
    if frame_end == -1:
        frame_end = target_motion.local_rotation.shape[0]
    local_rotation = target_motion.local_rotation[frame_beg:frame_end, ...]
    root_translation = target_motion.root_translation[frame_beg:frame_end, ...]
    state = SkeletonState.from_rotation_and_root_translation(target_motion.skeleton_tree, local_rotation, root_translation, is_local=True)
    target_motion = SkeletonMotion.from_skeleton_state(state, fps=target_motion.fps)
    if hinges:
        target_motion = RM.project_joints(target_motion)
    out['hinge_rotation'] = target_motion.local_rotation.clone()
    local_rotation = target_motion.local_rotation
    root_translation = target_motion.root_translation
    min_h = torch.min(target_motion.global_translation[..., 2])
    out['min_h'] = min_h.clone()
    root_translation[:, 2] += -min_h
    root_translation[:, 2] += cfg['root_height_offset']
    state = SkeletonState.from_rotation_and_root_translation(target_motion.skeleton_tree, local_rotation, root_translation, is_local=True)
    target_motion = SkeletonMotion.from_skeleton_state(state, fps=target_motion.fps)
    out.update(rotation=target_motion.local_rotation.clone(), root_translation=target_motion.root_translation.clone(),
               global_velocity=target_motion.global_velocity.clone(), global_angular_velocity=target_motion.global_angular_velocity.clone())
    assert all(v.dtype == torch.float32 for v in out.values())
    return out, target_motion


def clip_inputs(motion):
    return {'rotation': motion.rotation.clone(), 'root_translation': motion.root_translation.clone(), 'fps': motion.fps,
            'is_local': bool(motion.is_local)}


def as_global(motion, tmp):
    """The motion re-saved by poselib in global form, read back."""
    m = SkeletonMotion.from_skeleton_state(motion.global_repr(), fps=motion.fps)
    path = os.path.join(tmp, 'global.npy')
    m.to_file(path)
    m = SkeletonMotion.from_file(path)
    assert not m.is_local
    return m


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    for f in DATA_FILES:
        shutil.copyfile(os.path.join(POSELIB, 'data', f), os.path.join(OUT_DIR, f))
    for f in CONFIGS:
        shutil.copyfile(os.path.join(POSELIB, 'data', 'configs', f), os.path.join(OUT_DIR, f))
    cfgs = {f: json.load(open(os.path.join(OUT_DIR, f))) for f in CONFIGS}
    cmu_cfg, sfu_cfg = cfgs[CONFIGS[0]], cfgs[CONFIGS[1]]
    load = lambda f: SkeletonState.from_file(os.path.join(OUT_DIR, f))
    amp = load('amp_humanoid_tpose.npy')
    avatar_tree = SkeletonMotion.from_file(os.path.join(CLIP_DIR, 'RL_Avatar_TurnLeft90_Motion.npy')).skeleton_tree
    avatar = SkeletonState.zero_pose(avatar_tree)
    topo_cfg = dict(cmu_cfg, joint_mapping=dict(cmu_cfg['joint_mapping'], LeftHand='shield', LeftFingerBase='left_hand'))
    tmp = tempfile.mkdtemp()
    cmu_specs = [(2, 120, 11, (-1, -1)), (18, 60, 16, (-1, -1)), (40, 30, 13, (5, 33))]
    sfu_specs = [(3, 30, 21, (-1, -1)), (17, 60, 22, (-1, -1))]

    def case(tpose_file, cfg, cfg_file, specs, target, target_name, hinges=True, to_global=False):
        clips, outs = [], []
        for frames, fps, seed, trim in specs:
            tpose = load(tpose_file)                       # a fresh tree per clip: keep_nodes_by_names edits offsets in place
            motion = synthesize(tpose, frames, fps, seed, cfg['scale'])
            if to_global:
                motion = as_global(motion, tmp)
            offsets = target.skeleton_tree.local_translation.clone()
            out, _ = run_reference(motion, load(tpose_file), target, cfg, trim, hinges)
            assert torch.equal(offsets, target.skeleton_tree.local_translation), 'the target tree was edited'
            clips.append(clip_inputs(motion))
            outs.append(out)
        return {'source_tpose': tpose_file, 'target': target_name, 'config': cfg_file, 'joint_mapping': cfg['joint_mapping'],
                'rotation': cfg['rotation'], 'scale': cfg['scale'], 'root_height_offset': cfg['root_height_offset'],
                'hinges': hinges, 'clips': clips, 'trims': [s[3] for s in specs], 'outputs': outs}

    G = {'cmu': case('cmu_tpose.npy', cmu_cfg, CONFIGS[0], cmu_specs, amp, 'amp_humanoid_tpose.npy'),
         'sfu': case('sfu_tpose.npy', sfu_cfg, CONFIGS[1], sfu_specs, amp, 'amp_humanoid_tpose.npy'),
         'global': case('cmu_tpose.npy', cmu_cfg, CONFIGS[0], cmu_specs[1:2], amp, 'amp_humanoid_tpose.npy', to_global=True),
         'unmapped': case('cmu_tpose.npy', cmu_cfg, CONFIGS[0], cmu_specs[1:2], avatar, 'RL_Avatar_TurnLeft90_Motion.npy'),
         'nohinge': case('cmu_tpose.npy', cmu_cfg, CONFIGS[0], cmu_specs, amp, 'amp_humanoid_tpose.npy', hinges=False),
         'topology': case('cmu_tpose.npy', topo_cfg, None, cmu_specs[1:2], avatar, 'RL_Avatar_TurnLeft90_Motion.npy')}
    shutil.rmtree(tmp)
    path = os.path.join(ROOT, 'tests', 'golden', 'retarget.pt')
    torch.save(G, path)
    print('wrote', path, '%.1f KB' % (os.path.getsize(path) / 1e3))

    if '--time' in sys.argv:                               # the reference pipeline on this CPU, one clip at a time
        rows = []
        for label, frames in (('64 x 40 frames', 40), ('64 x 300 frames', 300)):
            motions = [synthesize(load('cmu_tpose.npy'), frames, 30, 100 + i, cmu_cfg['scale']) for i in range(64)]
            t0 = time.perf_counter()
            for m in motions:
                run_reference(m, load('cmu_tpose.npy'), amp, cmu_cfg, (-1, -1))
            rows.append({'what': 'reference pipeline (poselib, CPU, f32), T-pose load included', 'clips': label,
                         'seconds': round(time.perf_counter() - t0, 3), 'torch_threads': torch.get_num_threads()})
            print(rows[-1])
        with open(os.path.join(ROOT, 'profiles', 'retarget.jsonl'), 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
