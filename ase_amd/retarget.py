"""Motion retargeting on the device: poselib's ``retarget_motion.py`` and ``SkeletonState.retarget_to`` - a
mocap clip on its own skeleton (CMU, SFU, ...) -> a ``SkeletonMotion`` of the humanoid - for any number of clips in seven
launches (``ase_hip_retarget_*``, csrc/retarget.hip), without poselib or scipy.

The host reads files, matches joint NAMES and builds integer tables once, in the constructor; it does no quaternion
arithmetic.  The T-poses go through the same device routines as the motion, in one-frame calls.  Stages, as the reference:
pose transfer (``retarget_to_by_tpose``), trim (a frame range per clip, applied as table arithmetic), hinge projection
(``project_joints``, from a table of limbs), grounding (per-clip minimum of global z), velocities
(``SkeletonMotion.from_skeleton_state``).  Everything is f64 on the device and rounded to f32 once, at the store of the
four arrays of a clip file.

``_get_pairwise_average_translation`` (skeleton3d.py:694-704) is NOT computed: it only feeds the offsets of the reduced
source tree, which ``retarget_to`` discards - the result lives on the target T-pose's own tree.

Not here: FBX / MJCF import, plotting, ``crop`` with an fps change.
"""
import json
import os

import numpy as np
import torch

MAX_BODIES = 64

# project_joints (poselib/retarget_motion.py:24-175) as a table: a limb is (upper, lower, end, bend sign, twist sense).  The
# lower body becomes a hinge about y bent by sign * |theta|; the upper body takes the twist about the offset of `end`, positive
# where dir0.y <= 0 (sense -1) or dir0.y >= 0 (sense +1).  `identity` bodies are set to the identity rotation.
AMP_HUMANOID_HINGES = {
    'limbs': (('right_upper_arm', 'right_lower_arm', 'right_hand', -1, -1),
              ('left_upper_arm', 'left_lower_arm', 'left_hand', -1, -1),
              ('right_thigh', 'right_shin', 'right_foot', +1, +1),
              ('left_thigh', 'left_shin', 'left_foot', +1, +1)),
    'identity': ('left_hand', 'right_hand'),
}


def read_tpose(path):
    """One ``SkeletonState`` file as poselib writes it, in local or global form -> dict: rotation [B, 4], root_translation [3]
    (f64), parent_indices [B], local_translation [B, 3] (f32), node_names, is_local.  Nothing is computed.  The format is a
    PICKLE: read trusted files only."""
    try:
        d = np.load(path, allow_pickle=True).item()
    except (ValueError, AttributeError, EOFError) as e:
        raise ValueError(f'{path}: not a SkeletonState file ({e})') from e
    if not isinstance(d, dict) or d.get('__name__') != 'SkeletonState':
        name = d.get('__name__') if isinstance(d, dict) else type(d).__name__
        raise ValueError(f"{path}: holds a {name!r}, not a 'SkeletonState'")
    tree = d['skeleton_tree']
    arr = lambda x, dt: np.ascontiguousarray(np.asarray(x['arr']), dtype=dt)
    s = {'rotation': arr(d['rotation'], np.float64), 'root_translation': arr(d['root_translation'], np.float64),
         'parent_indices': arr(tree['parent_indices'], np.int64), 'local_translation': arr(tree['local_translation'], np.float32),
         'node_names': [str(x) for x in tree['node_names']], 'is_local': bool(d['is_local'])}
    B = len(s['node_names'])
    if s['rotation'].shape != (B, 4) or s['root_translation'].shape != (3,) or s['parent_indices'].shape != (B,) or \
            s['local_translation'].shape != (B, 3):
        raise ValueError(f'{path}: array shapes do not describe one pose of {B} bodies')
    return s


def zero_pose(node_names, parent_indices, local_translation, root_translation=(0.0, 0.0, 0.0)):
    """``SkeletonState.zero_pose`` of a tree, in ``read_tpose``'s form."""
    B = len(node_names)
    rot = np.zeros((B, 4), dtype=np.float64)
    rot[:, 3] = 1.0
    return {'rotation': rot, 'root_translation': np.asarray(root_translation, dtype=np.float64),
            'parent_indices': np.asarray(parent_indices, dtype=np.int64),
            'local_translation': np.ascontiguousarray(local_translation, dtype=np.float32),
            'node_names': [str(x) for x in node_names], 'is_local': True}


def tree_table(parent_indices, what='skeleton'):
    """The device form of a tree -> int32 [B, max depth + 2]: column 0 the depth of a body, then its chain from the root down
    to itself (padded with -1).  Refuses a parent that does not precede its child."""
    parents = [int(p) for p in parent_indices]
    chains = []
    for b, p in enumerate(parents):
        if not (-1 <= p < b) or (b == 0 and p != -1):
            raise ValueError(f'{what}: parent {p} of body {b} does not precede it')
        chains.append(([] if p < 0 else chains[p]) + [b])
    ld = max(len(c) for c in chains) + 1
    tab = np.full((len(parents), ld), -1, dtype=np.int32)
    for b, c in enumerate(chains):
        tab[b, 0] = len(c) - 1
        tab[b, 1:1 + len(c)] = c
    return tab


def _reduced_tree(names, parents, keep, what):
    """``SkeletonTree.keep_nodes_by_names`` (skeleton3d.py:212-259) without the offsets -> (kept body indices in tree order,
    the parent of each among the kept ones, -1 for a root)."""
    kept = [b for b, n in enumerate(names) if n in keep]
    pos = {b: i for i, b in enumerate(kept)}
    red_parent = []
    for b in kept:
        p = int(parents[b])
        dropped = False
        while p != -1 and p not in pos:
            p, dropped = int(parents[p]), True
        if p == -1 and dropped:
            raise ValueError(f'{what}: the root {names[0]!r} is not in the joint mapping (the root node cannot be dropped)')
        red_parent.append(-1 if p == -1 else pos[p])
    return kept, red_parent


def mapping_tables(src_names, src_parents, tgt_names, tgt_parents, joint_mapping):
    """The integer tables of ``ase_hip_retarget_chain`` / ``_pose`` from the joint names -> dict of int32 arrays: rs_body,
    rs_parent, rt_src, rt_tree, rt_body, ancestor.  Refuses what ``SkeletonState._remapped_to`` asserts on."""
    src_names, tgt_names = [str(x) for x in src_names], [str(x) for x in tgt_names]
    mapping = {str(k): str(v) for k, v in joint_mapping.items()}
    inv = {v: k for k, v in mapping.items()}
    rs_body, rs_parent = _reduced_tree(src_names, src_parents, set(mapping), 'source skeleton')
    rt_body, rt_parent = _reduced_tree(tgt_names, tgt_parents, set(inv), 'target skeleton')
    if not (len(mapping) == len(rs_body) == len(rt_body)) or not rs_body:
        raise ValueError(f'joint mapping of {len(mapping)} pairs: the reduced trees have different sizes ({len(rs_body)} source, '
                         f'{len(rt_body)} target bodies) - the joint mapping is not consistent with the skeleton trees')
    rs_index = {src_names[b]: m for m, b in enumerate(rs_body)}
    rt_index = {tgt_names[b]: i for i, b in enumerate(rt_body)}
    rt_src = [rs_index[inv[tgt_names[b]]] for b in rt_body]
    ancestor = []
    for b in range(len(tgt_names)):                      # STEP 5: a body outside the mapping takes its nearest mapped ancestor
        k = b
        while tgt_names[k] not in rt_index:
            k = int(tgt_parents[k])
            if k < 0:
                raise ValueError(f'target body {tgt_names[b]!r} has no mapped ancestor')
        ancestor.append(rt_index[tgt_names[k]])
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return {'rs_body': i32(rs_body), 'rs_parent': i32(rs_parent), 'rt_src': i32(rt_src),
            'rt_tree': tree_table(rt_parent, 'reduced target tree'), 'rt_body': i32(rt_body), 'ancestor': i32(ancestor)}


def hinge_roles(node_names, hinges):
    """The roles table of ``ase_hip_retarget_hinge`` -> int32 [B, 6] = (role, upper, lower, end, bend sign, twist sense)."""
    names = [str(x) for x in node_names]
    roles = np.zeros((len(names), 6), dtype=np.int32)

    def index(n):
        if n not in names:
            raise ValueError(f'hinges: the target skeleton has no body {n!r}')
        return names.index(n)
    for upper, lower, end, bend, twist in hinges['limbs']:
        if bend not in (-1, 1) or twist not in (-1, 1):
            raise ValueError(f'hinges: bend sign {bend!r} / twist sense {twist!r} of {upper!r} (+1 or -1)')
        u, l, e = index(upper), index(lower), index(end)
        roles[u] = (2, u, l, e, bend, twist)
        roles[l] = (3, u, l, e, bend, twist)
    for n in hinges.get('identity', ()):
        roles[index(n)] = (1, 0, 0, 0, 0, 0)
    return roles


def _frame_tables(num_frames):
    n = np.asarray(num_frames, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(n)[:-1]])
    return first.astype(np.int32), n.astype(np.int32), np.repeat(np.arange(len(n), dtype=np.int32), n)


class Retargeter:
    """``retarget_motion.main()`` (poselib/retarget_motion.py:178-251) for a list of clips.  ``source_tpose`` / ``target_tpose``:
    ``read_tpose`` dicts; ``joint_mapping``: source name -> target name; ``rotation``: xyzw, the root rotation from the source to
    the target skeleton; ``hinges``: the table of ``project_joints`` (None skips that stage).  All tables are built and uploaded
    here, and the T-poses are taken through the device routines once."""

    def __init__(self, backend, device, source_tpose, target_tpose, joint_mapping, rotation, scale, root_height_offset=0.0,
                 hinges=AMP_HUMANOID_HINGES, trim=None):
        self.be, self.device = backend, torch.device(device)
        self.source, self.target = source_tpose, target_tpose
        Bs, Bt = len(source_tpose['node_names']), len(target_tpose['node_names'])
        for what, B in (('source', Bs), ('target', Bt)):
            if not 1 <= B <= MAX_BODIES:
                raise ValueError(f'{what} skeleton: {B} bodies (1-{MAX_BODIES})')
        if len(rotation) != 4:
            raise ValueError(f'rotation {rotation!r}: a quaternion xyzw')
        self.trim = trim
        i32 = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32).to(self.device)
        f64 = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).to(self.device)
        self.src_tree = i32(tree_table(source_tpose['parent_indices'], 'source skeleton'))
        self.tgt_tree = i32(tree_table(target_tpose['parent_indices'], 'target skeleton'))
        tabs = mapping_tables(source_tpose['node_names'], source_tpose['parent_indices'], target_tpose['node_names'],
                              target_tpose['parent_indices'], joint_mapping)
        self.tabs = {k: i32(v) for k, v in tabs.items()}
        self.tgt_parent = i32(target_tpose['parent_indices'])
        self.tgt_offsets = torch.as_tensor(target_tpose['local_translation'], dtype=torch.float32).contiguous().to(self.device)
        self.roles = None if hinges is None else i32(hinge_roles(target_tpose['node_names'], hinges))
        # (the reference reads the config's rotation with torch.tensor(list): an f32 tensor, whatever the data's dtype)
        self.params = f64(np.concatenate([np.asarray(rotation, dtype=np.float32).astype(np.float64), source_tpose['root_translation'],
                                          target_tpose['root_translation'], [float(scale), float(root_height_offset)]]))
        # the T-poses: one-frame calls of the motion's own routines
        one = tuple(i32(x) for x in ([0], [1], [0], [0]))
        mode = lambda s: 0 if s['is_local'] else 2
        g = backend.retarget_fk(f64(source_tpose['rotation'][None]), mode(source_tpose), self.src_tree, *one)
        t = self.tabs
        self.tpose_global = backend.retarget_chain(g, t['rs_body'], t['rs_parent'], t['rt_src'], t['rt_tree'], self.params)[0].contiguous()
        self.target_global = backend.retarget_fk(f64(target_tpose['rotation'][None]), mode(target_tpose), self.tgt_tree, *one)[0].contiguous()

    @classmethod
    def from_config(cls, json_path, data_dir, backend, device, hinges=AMP_HUMANOID_HINGES):
        """A retarget config of the reference (poselib/data/configs/retarget_*_to_amp.json), keys as they are: source_tpose,
        target_tpose (their base names are looked up in ``data_dir``), joint_mapping, rotation, scale, root_height_offset,
        trim_frame_beg, trim_frame_end (-1: the clip's own end).  source_motion / target_motion_path are kept in ``config``."""
        with open(json_path) as f:
            cfg = json.load(f)
        tpose = lambda k: read_tpose(os.path.join(data_dir, os.path.basename(cfg[k])))
        r = cls(backend, device, tpose('source_tpose'), tpose('target_tpose'), cfg['joint_mapping'], cfg['rotation'], cfg['scale'],
                root_height_offset=cfg.get('root_height_offset', 0.0), hinges=hinges,
                trim=(int(cfg.get('trim_frame_beg', -1)), int(cfg.get('trim_frame_end', -1))))
        r.config = cfg
        return r

    def _ranges(self, frames, trim):
        trim = self.trim if trim is None else trim
        if trim is None:
            trim = (-1, -1)
        if len(trim) == 2 and not isinstance(trim[0], (tuple, list)):
            trim = [trim] * len(frames)
        if len(trim) != len(frames):
            raise ValueError(f'trim: {len(trim)} ranges for {len(frames)} clips')
        out = []
        for c, (F, (beg, end)) in enumerate(zip(frames, trim)):                 # retarget_motion.py:211-223, a python slice
            beg, end = (0 if beg == -1 else int(beg)), (F if end == -1 else int(end))
            if beg < 0 or end < 0:
                raise ValueError(f'clip {c}: trim range [{beg}, {end}) (-1 or a frame index)')
            beg, end = min(beg, F), min(end, F)
            if end - beg < 2:
                raise ValueError(f'clip {c}: {max(end - beg, 0)} frame(s) after trimming {F} to [{beg}, {end}); a clip has 2 or more')
            out.append((beg, end))
        return out

    def retarget(self, clips, trim=None):
        """``clips``: a list of clip dicts in ``read_clip``'s form on the SOURCE skeleton (``read_clip(path, allow_global=True)``;
        arrays numpy or torch; ``global_velocity`` / ``global_angular_velocity`` are not needed), all local or all global.
        ``trim``: (beg, end) for every clip or one pair per clip, -1 as in the config; None: the constructor's.
        -> a list of clip dicts on the target skeleton; rotation [F, B, 4], root_translation [F, 3], global_velocity,
        global_angular_velocity [F, B, 3] are f32 tensors on the device (views of one allocation per array)."""
        be = self.be
        if not clips:
            raise ValueError('retarget: no clips')
        Bs = len(self.source['node_names'])
        local = [bool(c.get('is_local', True)) for c in clips]
        if any(x != local[0] for x in local):
            raise ValueError('retarget: clips in local and in global form in one call')
        up = lambda x: torch.as_tensor(x).to(self.device, dtype=torch.float64)
        rots, roots = [up(c['rotation']) for c in clips], [up(c['root_translation']) for c in clips]
        for c, (clip, r, t) in enumerate(zip(clips, rots, roots)):
            if r.dim() != 3 or r.shape[1:] != (Bs, 4) or t.shape != (r.shape[0], 3):
                raise ValueError(f'clip {c}: rotation {tuple(r.shape)} / root_translation {tuple(t.shape)} do not describe frames of the '
                                 f'{Bs} source bodies')
            if 'parent_indices' in clip and not np.array_equal(np.asarray(clip['parent_indices']), self.source['parent_indices']):
                raise ValueError(f'clip {c}: skeleton differs from the source T-pose')
            if not float(clip['fps']) > 0:
                raise ValueError(f"clip {c}: fps {clip['fps']!r}")
        frames = [int(r.shape[0]) for r in rots]
        ranges = self._ranges(frames, trim)
        src_start = np.concatenate([[0], np.cumsum(frames)[:-1]])
        first, num, frame_clip = _frame_tables([e - b for b, e in ranges])
        i32 = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32).to(self.device)
        first_d, num_d, frame_clip_d = i32(first), i32(num), i32(frame_clip)
        src_first = i32(src_start + np.asarray([b for b, _ in ranges]))
        fps = torch.tensor([float(c['fps']) for c in clips], dtype=torch.float64).to(self.device)
        rot, root = torch.cat(rots).contiguous(), torch.cat(roots).contiguous()
        t = self.tabs
        maps = (first_d, num_d, src_first, frame_clip_d)
        g = be.retarget_fk(rot, 0 if local[0] else 1, self.src_tree, *maps)
        g = be.retarget_chain(g, t['rs_body'], t['rs_parent'], t['rt_src'], t['rt_tree'], self.params)
        lr, rt = be.retarget_pose(g, self.tpose_global, self.target_global, root, self.params, t['rt_body'], t['ancestor'],
                                  self.tgt_parent, *maps)
        if self.roles is not None:
            lr = be.retarget_hinge(lr, rt, self.tgt_offsets, self.tgt_tree, self.roles)
        min_z = be.retarget_ground(lr, rt, self.tgt_offsets, self.tgt_tree, first_d, num_d)
        gr, gt, rot_out, root_out = be.retarget_finish(lr, rt, min_z, self.params, self.tgt_offsets, self.tgt_tree, frame_clip_d)
        vel, ang = be.retarget_velocity(gr, gt, first_d, num_d, fps, frame_clip_d)
        out = []
        for c, clip in enumerate(clips):
            s = slice(int(first[c]), int(first[c]) + int(num[c]))
            out.append({'rotation': rot_out[s], 'root_translation': root_out[s], 'global_velocity': vel[s],
                        'global_angular_velocity': ang[s], 'parent_indices': np.asarray(self.target['parent_indices'], dtype=np.int64),
                        'local_translation': np.asarray(self.target['local_translation'], dtype=np.float32),
                        'node_names': list(self.target['node_names']), 'fps': float(clip['fps']), 'is_local': True})
        return out
