"""Motion clips on the device: the reference's ``MotionLib`` (utils/motion_lib.py) - loader, sampling and
state interface - and ``HumanoidAMP.fetch_amp_obs_demo`` / ``build_amp_obs_demo`` (env/tasks/humanoid_amp.py:63-105) over
clip arrays resident in HBM.

Loading (``DeviceMotionLib.from_file``): the host READS the files - a dataset ``.yaml`` or one ``.npy`` clip, poselib's
``SkeletonMotion`` dictionaries, with numpy / yaml only - checks them, concatenates the raw f64 arrays of all clips and
uploads them once; it does no arithmetic on frames.  One HIP launch (``ase_hip_clip_frames``) then computes what
``MotionLib._load_motions`` leaves in ``ml.gts, ml.grs, ml.lrs, ml.grvs, ml.gravs, ml.dvs``: the forward-kinematics chain of
every frame (global rotation / translation of every body) and the joint velocities from consecutive frames, in f64 as poselib
does, stored f32.  ``from_reference`` takes a loaded reference ``MotionLib`` instead, ``from_arrays`` the arrays themselves.

Sampling: everything per sample - frame blend, slerp of the root and every local rotation, exponential-map dof positions,
key-body interpolation, then the 140-float observation frame (root height, tangent-normal root rotation, local velocities,
dof observations, key bodies) - runs in two HIP kernels (``ase_hip_motion_state``, ``ase_hip_build_amp_obs``).
``AmpObsDemoSource.fetch_into`` is the whole demo fetch - draws, sampler, frames and the store into the demo ring - as one
launch (``ase_hip_amp_demo_fetch``, N11).

There is no host fallback for either.  ``DeviceMotionLib.from_clips`` takes clip dicts instead of files (``read_clip``'s form,
arrays on the host or on the device - what ``ase_amd.retarget.Retargeter.retarget`` returns), ``write_clip`` writes one as a
poselib ``SkeletonMotion`` file.  Not here: FBX / MJCF import; the motion library itself loads local-rotation clips only
(``read_clip(path, allow_global=True)`` reads a global-rotation clip for the retargeter).
"""
import os
from collections import OrderedDict

import numpy as np
import torch


def fetch_motion_files(motion_file):
    """MotionLib._fetch_motion_files (utils/motion_lib.py:238-261) -> (files, weights): a ``.yaml`` lists ``motions: [{file,
    weight}]`` with files relative to its own directory; anything else is one clip of weight 1.  The path is taken as given."""
    motion_file = os.fspath(motion_file)
    if os.path.splitext(motion_file)[1] != '.yaml':
        return [motion_file], [1.0]
    import yaml
    with open(motion_file, 'r') as f:
        cfg = yaml.load(f, Loader=yaml.SafeLoader)
    if not isinstance(cfg, dict) or not cfg.get('motions'):
        raise ValueError(f"{motion_file}: no 'motions' list")
    dir_name = os.path.dirname(motion_file)
    files, weights = [], []
    for entry in cfg['motions']:
        w = float(entry['weight'])
        if not w >= 0:
            raise ValueError(f"{motion_file}: weight {entry['weight']!r} of {entry['file']} is negative")
        files.append(os.path.join(dir_name, entry['file']))
        weights.append(w)
    if not sum(weights) > 0:
        raise ValueError(f'{motion_file}: all weights are zero')
    return files, weights


def read_clip(path, allow_global=False):
    """One ``SkeletonMotion`` file as poselib writes it (``numpy.save`` of an ordered dict, arrays under ``['arr']``) -> dict of
    numpy arrays: rotation [F, J, 4], root_translation [F, 3], global_velocity / global_angular_velocity [F, J, 3] (f64),
    parent_indices [J], local_translation [J, 3] (f32), fps, is_local.  Nothing is computed.  A clip that stores GLOBAL rotations
    is refused unless ``allow_global`` (the retargeter takes one; the motion library does not).

    The format is a PICKLE (``allow_pickle=True``): loading a file runs code it names.  Read trusted files only."""
    try:
        d = np.load(path, allow_pickle=True).item()
    except (ValueError, AttributeError, EOFError) as e:
        raise ValueError(f'{path}: not a SkeletonMotion file ({e})') from e
    if not isinstance(d, dict) or d.get('__name__') != 'SkeletonMotion':
        name = d.get('__name__') if isinstance(d, dict) else type(d).__name__
        raise ValueError(f"{path}: holds a {name!r}, not a 'SkeletonMotion'")
    if not d['is_local'] and not allow_global:
        raise ValueError(f'{path}: the clip stores global rotations (is_local == False), which are not loaded; '
                         're-save it in local form (rotations relative to the parent body, is_local == True)')
    tree = d['skeleton_tree']
    arr = lambda x, dt: np.ascontiguousarray(np.asarray(x['arr']), dtype=dt)
    c = {'rotation': arr(d['rotation'], np.float64), 'root_translation': arr(d['root_translation'], np.float64),
         'global_velocity': arr(d['global_velocity'], np.float64),
         'global_angular_velocity': arr(d['global_angular_velocity'], np.float64),
         'parent_indices': arr(tree['parent_indices'], np.int64), 'local_translation': arr(tree['local_translation'], np.float32),
         'node_names': list(tree['node_names']), 'fps': float(d['fps']), 'is_local': bool(d['is_local'])}
    F, J = c['rotation'].shape[:2]
    if c['rotation'].shape != (F, J, 4) or c['root_translation'].shape != (F, 3) or c['global_velocity'].shape != (F, J, 3) or \
            c['global_angular_velocity'].shape != (F, J, 3) or c['parent_indices'].shape != (J,) or c['local_translation'].shape != (J, 3):
        raise ValueError(f'{path}: array shapes do not describe {F} frames of {J} bodies')
    if F < 2:
        raise ValueError(f'{path}: {F} frame(s); a clip has 2 or more')
    if not c['fps'] > 0:
        raise ValueError(f"{path}: fps {d['fps']!r}")
    for b, p in enumerate(c['parent_indices']):
        if not (-1 <= p < b) or (b == 0 and p != -1):
            raise ValueError(f'{path}: parent {p} of body {b} does not precede it')
    return c


def write_clip(path, clip):
    """A clip dict (``read_clip``'s form; arrays numpy or torch, on any device) as the ``SkeletonMotion`` file poselib's
    ``to_file`` writes - ``numpy.save`` of an ordered dict with the keys, key order and dtypes of the shipped clip files (f64
    arrays, int64 parents, f32 offsets) - which ``read_clip`` and the reference's ``SkeletonMotion.from_file`` load."""
    def host(x, dt):
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        return np.ascontiguousarray(x, dtype=dt)

    def entry(x, dt):
        return {'arr': host(x, dt), 'context': {'dtype': np.dtype(dt).name}}
    F, J = host(clip['rotation'], np.float64).shape[:2]
    for k, shape in (('rotation', (F, J, 4)), ('root_translation', (F, 3)), ('global_velocity', (F, J, 3)),
                     ('global_angular_velocity', (F, J, 3)), ('parent_indices', (J,)), ('local_translation', (J, 3))):
        if tuple(clip[k].shape) != shape:
            raise ValueError(f'{path}: {k} {tuple(clip[k].shape)}, expected {shape}')
    if len(clip['node_names']) != J:
        raise ValueError(f"{path}: {len(clip['node_names'])} node names for {J} bodies")
    tree = OrderedDict([('node_names', [str(n) for n in clip['node_names']]),
                        ('parent_indices', entry(clip['parent_indices'], np.int64)),
                        ('local_translation', entry(clip['local_translation'], np.float32))])
    d = OrderedDict([('rotation', entry(clip['rotation'], np.float64)), ('root_translation', entry(clip['root_translation'], np.float64)),
                     ('global_velocity', entry(clip['global_velocity'], np.float64)),
                     ('global_angular_velocity', entry(clip['global_angular_velocity'], np.float64)),
                     ('skeleton_tree', tree), ('is_local', bool(clip.get('is_local', True))), ('fps', float(clip['fps'])),
                     ('__name__', 'SkeletonMotion')])
    with open(path, 'wb') as f:                              # (numpy.save appends '.npy' to a bare path that lacks it)
        np.save(f, d, allow_pickle=True)


def clip_tables(clips, names, label, dof_body_ids, dof_offsets, key_body_ids):
    """Per-clip tables as ``MotionLib._load_motions`` (utils/motion_lib.py:192-228,82-85) and the raw arrays of ``clips``
    (``read_clip`` dicts; ``names`` label them in messages) concatenated along the frame axis - numpy when every clip's arrays
    are, torch tensors otherwise.  Raises ``ValueError`` for everything the loader refuses."""
    dof_body_ids, dof_offsets, key_body_ids = [int(x) for x in dof_body_ids], [int(x) for x in dof_offsets], [int(x) for x in key_body_ids]
    if len(dof_offsets) != len(dof_body_ids) + 1 or dof_offsets[0] != 0:
        raise ValueError(f'{label}: dof_offsets {dof_offsets} do not describe the {len(dof_body_ids)} joints of dof_body_ids')
    for j in range(len(dof_body_ids)):
        if dof_offsets[j + 1] - dof_offsets[j] not in (1, 3):
            raise ValueError(f'{label}: joint {j} has {dof_offsets[j + 1] - dof_offsets[j]} dofs (1 or 3 supported)')
    first = clips[0]
    J = first['rotation'].shape[1]
    for name, ids in (('dof_body_id', dof_body_ids), ('key_body_id', key_body_ids)):
        for b in ids:
            if not 0 <= b < J:
                raise ValueError(f'{names[0]}: {name} {b} outside the skeleton of {J} bodies')
    parents = np.asarray(first['parent_indices'])
    for f, c in zip(names, clips):
        if c['rotation'].shape[1] != J or not np.array_equal(np.asarray(c['parent_indices']), parents):
            raise ValueError(f"{f}: skeleton ({c['rotation'].shape[1]} bodies, parents {np.asarray(c['parent_indices']).tolist()}) differs from "
                             f'that of {names[0]}')
        if not c.get('is_local', True):
            raise ValueError(f'{f}: the clip stores global rotations (is_local == False), which are not loaded')
        if c['rotation'].shape[0] < 2:
            raise ValueError(f"{f}: {c['rotation'].shape[0]} frame(s); a clip has 2 or more")
    num_frames = [int(c['rotation'].shape[0]) for c in clips]
    fps = [float(c['fps']) for c in clips]
    starts = np.concatenate([[0], np.cumsum(num_frames)[:-1]])
    on_host = all(isinstance(c[k], np.ndarray) for c in clips for k in ('rotation', 'root_translation', 'global_velocity',
                                                                       'global_angular_velocity'))
    if on_host:
        cat = lambda k, sel=None: np.concatenate([c[k] if sel is None else c[k][:, sel] for c in clips], axis=0)
    else:
        cat = lambda k, sel=None: torch.cat([torch.as_tensor(c[k]) if sel is None else torch.as_tensor(c[k])[:, sel] for c in clips], dim=0)
    body0 = lambda k: np.ascontiguousarray(cat(k)[:, 0]) if on_host else cat(k, 0)
    return {'fps': fps, 'num_frames': num_frames,
            'dt': [1.0 / x for x in fps],                                                  # motion_lib.py:193
            'lengths': [1.0 / x * (n - 1) for x, n in zip(fps, num_frames)],               # motion_lib.py:196
            'length_starts': starts.tolist(),
            'frame_clip': np.repeat(np.arange(len(clips), dtype=np.int32), num_frames),
            'parent_indices': parents.tolist(),
            'rotation': cat('rotation'), 'root_translation': cat('root_translation'),
            'root_velocity': body0('global_velocity'),                                     # motion_lib.py:78-79: body 0
            'root_angular_velocity': body0('global_angular_velocity'),
            'local_translation': np.stack([np.asarray(c['local_translation'], dtype=np.float32) for c in clips]),   # each clip's own offsets
            'dof_body_ids': dof_body_ids, 'dof_offsets': dof_offsets, 'key_body_ids': key_body_ids}


def read_motion_files(motion_file, dof_body_ids, dof_offsets, key_body_ids):
    """The host side of ``DeviceMotionLib.from_file``: file list, per-clip tables as ``MotionLib._load_motions``
    (utils/motion_lib.py:192-228,82-85) and the raw arrays of all clips concatenated along the frame axis.  Raises
    ``ValueError`` naming the file for everything the loader refuses."""
    files, weights = fetch_motion_files(motion_file)
    _check_joint_tables(motion_file, dof_body_ids, dof_offsets)
    h = clip_tables([read_clip(f) for f in files], files, motion_file, dof_body_ids, dof_offsets, key_body_ids)
    h.update(motion_files=files, weights=weights)
    return h


def _check_joint_tables(label, dof_body_ids, dof_offsets):
    """The joint tables are checked before any file is read."""
    dof_body_ids, dof_offsets = [int(x) for x in dof_body_ids], [int(x) for x in dof_offsets]
    if len(dof_offsets) != len(dof_body_ids) + 1 or dof_offsets[0] != 0:
        raise ValueError(f'{label}: dof_offsets {dof_offsets} do not describe the {len(dof_body_ids)} joints of dof_body_ids')
    for j in range(len(dof_body_ids)):
        if dof_offsets[j + 1] - dof_offsets[j] not in (1, 3):
            raise ValueError(f'{label}: joint {j} has {dof_offsets[j + 1] - dof_offsets[j]} dofs (1 or 3 supported)')


def clip_cdf(weights):
    """The table of the device-side weighted clip choice (``ase_hip_amp_reset_due``, ``ase_hip_amp_demo_fetch``): ``cdf[m] = floor(2^24 cumsum(w)[m] /
    sum(w) + 0.5)`` taken in f64, the last entry ``2^24``; a 24-bit draw ``v`` picks the first clip with ``v < cdf[m]``, so clip
    m has probability ``(cdf[m] - cdf[m - 1]) / 2^24`` exactly and a clip of weight zero is never drawn.  -> int32 [n_clips]
    (the uint32 the kernel reads: no entry exceeds 2^24).  A positive weight whose interval comes out empty is refused."""
    w = np.asarray(torch.as_tensor(weights).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
    if w.size == 0 or not np.all(w >= 0) or not w.sum() > 0:
        raise ValueError(f'clip weights {w.tolist()}: non-negative with a positive sum')
    cdf = np.floor(2.0 ** 24 * np.cumsum(w) / w.sum() + 0.5).astype(np.int64)
    cdf[-1] = 1 << 24
    size = np.diff(cdf, prepend=0)
    for m in np.nonzero(w > 0)[0]:
        if size[m] <= 0:
            raise ValueError(f'clip {int(m)}: weight {w[m]:g} of {w.sum():g} is below the 2^-24 resolution of the device-side '
                             f'clip choice (it would never be drawn)')
    return torch.from_numpy(cdf.astype(np.int32))


class DeviceMotionLib:
    """``MotionLib`` (utils/motion_lib.py:57): same method names, argument meaning and return order."""

    CLIP_F32 = ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'dt')
    CLIP_I32 = ('num_frames', 'length_starts')

    def __init__(self, clips, backend, device, weights=None, generator=None):
        self.be, self._device, self.gen = backend, torch.device(device), generator
        self.clips = {k: clips[k].to(torch.float32).contiguous().to(self._device) for k in self.CLIP_F32}
        self.clips.update({k: clips[k].to(torch.int32).contiguous().to(self._device) for k in self.CLIP_I32})
        self.clips.update({k: [int(x) for x in clips[k]] for k in ('dof_body_ids', 'dof_offsets', 'key_body_ids')})
        self._motion_lengths = self.clips['lengths']
        n = self._motion_lengths.shape[0]
        w = torch.ones(n) if weights is None else torch.as_tensor(weights, dtype=torch.float32)
        self._motion_weights = (w / w.sum()).to(self._device)                 # motion_lib.py:213
        self.clip_cdf = clip_cdf(w / w.sum()).to(self._device)

    @classmethod
    def from_arrays(cls, clips, backend, device, **kw):
        return cls(clips, backend, device, **kw)

    @classmethod
    def from_clips(cls, clips, dof_body_ids, dof_offsets, key_body_ids, backend, device, weights=None, _names=None, _label='clips',
                   **kw):
        """The body of ``from_file`` behind the file reading: ``clips`` is a list of clip dicts in ``read_clip``'s form, with
        arrays on the host (numpy) or already on the device (torch - what ``Retargeter.retarget`` returns, so retargeted clips
        enter a motion library without touching the disk).  The raw arrays are concatenated, uploaded once as f64, and every
        frame array is computed by ONE launch of ``backend.clip_frames``.  ``fps`` is kept as an attribute."""
        clips = list(clips)
        if not clips:
            raise ValueError(f'{_label}: no clips')
        names = _names if _names is not None else [f'clip {i}' for i in range(len(clips))]
        h = clip_tables(clips, names, _label, dof_body_ids, dof_offsets, key_body_ids)
        dev = torch.device(device)
        up = lambda k, dt: (h[k] if isinstance(h[k], torch.Tensor) else torch.as_tensor(h[k], dtype=dt)).to(dev, dtype=dt).contiguous()
        out = backend.clip_frames(up('rotation', torch.float64), up('root_translation', torch.float64),
                                  up('root_velocity', torch.float64), up('root_angular_velocity', torch.float64),
                                  up('local_translation', torch.float32), h['parent_indices'], up('length_starts', torch.int32),
                                  up('num_frames', torch.int32), up('fps', torch.float64), up('frame_clip', torch.int32),
                                  h['dof_body_ids'], h['dof_offsets'])
        arrays = dict(zip(('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs'), out))
        arrays.update(lengths=torch.tensor(h['lengths'], dtype=torch.float32), dt=torch.tensor(h['dt'], dtype=torch.float32),
                      num_frames=torch.tensor(h['num_frames']), length_starts=torch.tensor(h['length_starts']),
                      dof_body_ids=h['dof_body_ids'], dof_offsets=h['dof_offsets'], key_body_ids=h['key_body_ids'])
        ml = cls(arrays, backend, dev, weights=weights, **kw)
        ml.fps = torch.tensor(h['fps'], dtype=torch.float32)
        return ml

    @classmethod
    def from_file(cls, motion_file, dof_body_ids, dof_offsets, key_body_ids, backend, device, **kw):
        """``MotionLib(motion_file, dof_body_ids, dof_offsets, key_body_ids, device)`` (utils/motion_lib.py:65-89): a dataset
        ``.yaml`` or one ``.npy`` clip.  The files are read on the host (``read_clip``; pickles - trusted files only) and handed
        to ``from_clips``: their raw f64 arrays uploaded once, every frame array computed by ONE launch of
        ``backend.clip_frames``.  ``motion_files`` and ``fps`` are kept as attributes.  Raises ``ValueError`` naming the file for
        what is refused."""
        files, weights = fetch_motion_files(motion_file)
        _check_joint_tables(motion_file, dof_body_ids, dof_offsets)
        kw.setdefault('weights', weights)
        ml = cls.from_clips([read_clip(f) for f in files], dof_body_ids, dof_offsets, key_body_ids, backend, device,
                            _names=files, _label=motion_file, **kw)
        ml.motion_files = files
        return ml

    @classmethod
    def from_reference(cls, ml, backend, device, dof_body_ids, dof_offsets, key_body_ids, **kw):
        """From a loaded reference ``MotionLib`` (any device): copies its frame arrays and per-clip tables."""
        clips = {'gts': ml.gts, 'grs': ml.grs, 'lrs': ml.lrs, 'grvs': ml.grvs, 'gravs': ml.gravs, 'dvs': ml.dvs,
                 'lengths': ml._motion_lengths, 'num_frames': ml._motion_num_frames, 'dt': ml._motion_dt,
                 'length_starts': ml.length_starts, 'dof_body_ids': dof_body_ids, 'dof_offsets': dof_offsets,
                 'key_body_ids': key_body_ids}
        kw.setdefault('weights', ml._motion_weights)
        return cls(clips, backend, device, **kw)

    def num_motions(self):
        return int(self._motion_lengths.shape[0])

    def get_total_length(self):
        return float(self._motion_lengths.sum())

    def get_motion_length(self, motion_ids):
        return self._motion_lengths[motion_ids]

    def sample_motions(self, n):
        """motion_lib.py:100-106."""
        return torch.multinomial(self._motion_weights, num_samples=n, replacement=True, generator=self.gen)

    def sample_time(self, motion_ids, truncate_time=None):
        """motion_lib.py:108-119: uniform phase times the (truncated) clip length."""
        phase = torch.rand(motion_ids.shape, device=self._device, generator=self.gen)
        motion_len = self._motion_lengths[motion_ids]
        if truncate_time is not None:
            assert truncate_time >= 0.0
            motion_len = motion_len - truncate_time
        return phase * motion_len

    def get_motion_state(self, motion_ids, motion_times):
        """motion_lib.py:122-172 -> (root_pos, root_rot, dof_pos, root_vel, root_ang_vel, dof_vel, key_pos)."""
        ids = motion_ids.to(torch.int32).contiguous()
        return self.be.motion_state(self.clips, ids, motion_times.to(torch.float32).contiguous())


class AmpObsDemoSource:
    """``HumanoidAMP.fetch_amp_obs_demo`` (env/tasks/humanoid_amp.py:63-84): ``num_samples`` demo observations of
    ``num_amp_obs_steps`` frames each, newest frame first, frame k taken ``k * dt`` before the sampled time."""

    def __init__(self, motion_lib, backend, num_amp_obs_steps=10, dt=1.0 / 30.0, local_root_obs=True, root_height_obs=True, seed=0):
        self._motion_lib, self.be = motion_lib, backend
        self._num_amp_obs_steps, self.dt = int(num_amp_obs_steps), float(dt)
        self._local_root_obs, self._root_height_obs = bool(local_root_obs), bool(root_height_obs)
        c = motion_lib.clips
        n_joints = len(c['dof_offsets']) - 1
        self._num_amp_obs_per_step = 13 + 6 * n_joints + c['dof_offsets'][-1] + 3 * len(c['key_body_ids'])   # humanoid_amp.py:107-118
        self._amp_obs_demo_buf = None
        # the Philox stream {seed, offset} of the device-side fetch (fetch_into); a call moves the offset on by one
        self.rng_state = torch.tensor([int(seed), 0], dtype=torch.int64, device=motion_lib._device)

    def get_num_amp_obs(self):
        return self._num_amp_obs_steps * self._num_amp_obs_per_step

    def fetch_into(self, out, ring_rows, head, n, *, motion_ids=None, motion_times0=None, advance=True, draws_out=None, head_dev=None):
        """``fetch_amp_obs_demo(n)`` written straight into rows ``(head + i) % ring_rows`` of ``out`` [ring_rows, >= steps *
        per_step] by ONE launch (``ase_hip_amp_demo_fetch``): no intermediate tensor, no staging buffer.  Without ``motion_ids`` /
        ``motion_times0`` the clips and times are drawn on the device, from ``clip_cdf`` and this source's ``rng_state`` (the
        draw table: include/ase_hip.h) - NOT the values a torch generator gives, which is why ``fetch_amp_obs_demo`` stays as it
        is.  With them (int32 / f32 [n]) the rows are bitwise ``build_amp_obs_demo(motion_ids, motion_times0)``."""
        ml = self._motion_lib
        truncate_time = self.dt * (self._num_amp_obs_steps - 1)
        drawn = motion_ids is None and motion_times0 is None
        self.be.amp_demo_fetch(ml.clips, out, ring_rows, head, n, self._num_amp_obs_steps, truncate_time, self.dt,
                               self._local_root_obs, self._root_height_obs, motion_ids=motion_ids, motion_times0=motion_times0,
                               rng_state=self.rng_state if drawn else None, clip_cdf=ml.clip_cdf if drawn else None,
                               advance=advance, draws_out=draws_out, head_dev=head_dev)

    def fetch_amp_obs_demo_device(self, num_samples):
        """``fetch_amp_obs_demo`` with the draws on the device -> a fresh [num_samples, steps * per_step] tensor."""
        out = torch.empty(num_samples, self.get_num_amp_obs(), dtype=torch.float32, device=self._motion_lib._device)
        self.fetch_into(out, num_samples, 0, num_samples)
        return out

    def fetch_amp_obs_demo(self, num_samples):
        ml = self._motion_lib
        motion_ids = ml.sample_motions(num_samples)
        # negative offsets are added in build_amp_obs_demo: shift the times into [truncate_time, end of clip]
        truncate_time = self.dt * (self._num_amp_obs_steps - 1)
        motion_times0 = ml.sample_time(motion_ids, truncate_time=truncate_time)
        motion_times0 = motion_times0 + truncate_time
        return self.build_amp_obs_demo(motion_ids, motion_times0).view(num_samples, self.get_num_amp_obs())

    def build_amp_obs_demo(self, motion_ids, motion_times0):
        """humanoid_amp.py:86-101 -> [n, steps, per_step] (a fresh buffer per call size, reused between calls)."""
        n, S = motion_ids.shape[0], self._num_amp_obs_steps
        dev = motion_times0.device
        ids = motion_ids.view(-1, 1).expand(n, S).reshape(-1)
        time_steps = -self.dt * torch.arange(0, S, device=dev)
        times = (motion_times0.unsqueeze(-1) + time_steps).reshape(-1)
        root_pos, root_rot, dof_pos, root_vel, root_ang_vel, dof_vel, key_pos = self._motion_lib.get_motion_state(ids, times)
        if self._amp_obs_demo_buf is None or self._amp_obs_demo_buf.shape[0] != n * S:
            self._amp_obs_demo_buf = torch.zeros(n * S, 1, self._num_amp_obs_per_step, device=dev, dtype=torch.float32)
        self.be.build_amp_obs(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_pos,
                              self._motion_lib.clips['dof_offsets'], self._local_root_obs, self._root_height_obs,
                              self._amp_obs_demo_buf, shift=False)
        return self._amp_obs_demo_buf.view(n, S, self._num_amp_obs_per_step)
