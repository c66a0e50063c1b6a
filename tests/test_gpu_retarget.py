"""The retargeter on the MI355X: ``ase_amd.retarget.Retargeter`` -> ``ase_hip_retarget_*`` against the f64
restatement of the reference's pipeline (tests/ref_retarget.py) evaluated on the stored inputs of tests/golden/retarget.pt.

Bounds (tests/ref_retarget.py ``bound``; derived as in tests/test_gpu_motion_load.py): the kernels and the restatement differ by
libm's f64 sqrt / acos / sin / cos and then one rounding to f32 - ulp_f32(ref) + 1e-12 for local rotations and the root
translation, + 6e-8 for rotations behind the hinge stage (an angle through acos next to its clamp: an argument error of
16 x 2^-53 moves it by at most sqrt(2 delta) = 6e-8 rad), + 1e-12 / dt for the velocity, + 6e-8 / dt for the angular velocity
(the filter is a convex combination).  Every launch writes into a window of a NaN-filled allocation whose guards are checked
after the call."""
import os

import numpy as np
import pytest
import torch

from ase_amd import lib as L
from ase_amd import retarget as RT
from ase_amd.motion_lib import DeviceMotionLib, read_clip, write_clip
from tests import emu_motion_load as EM
from tests import emu_retarget as E
from tests import ref_retarget as R
from tests.test_retarget_ref import CASES, OUTPUTS, RUN_ARGS, check_outputs

pytestmark = pytest.mark.gpu
GUARD = 64
METHODS = ('retarget_fk', 'retarget_chain', 'retarget_pose', 'retarget_hinge', 'retarget_ground', 'retarget_finish',
           'retarget_velocity')


class Guarded:
    """A HipBackend whose retarget_* launches write into windows of NaN-filled allocations (``out=``); ``check`` asserts that
    every guard element is still NaN and every window was written (no NaN left inside)."""

    def __init__(self, be):
        self.be, self.buffers, self.launches = be, [], []

    def __getattr__(self, name):
        fn = getattr(self.be, name)
        if name not in METHODS:
            return fn

        def call(*args, **kw):
            plain = fn(*args)
            plain = plain if isinstance(plain, tuple) else (plain,)
            outs = []
            for p in plain:
                flat = torch.full((p.numel() + 2 * GUARD,), float('nan'), dtype=p.dtype, device=p.device)
                outs.append(flat[GUARD:GUARD + p.numel()].view(p.shape))
                self.buffers.append((name, flat, p.numel()))
            res = fn(*args, out=tuple(outs) if len(outs) > 1 else outs[0])
            for p, o in zip(plain, res if isinstance(res, tuple) else (res,)):
                EM.bits_equal(p, o)                                        # a launch is deterministic
            self.launches.append(name)
            return res
        return call

    def check(self):
        torch.cuda.synchronize()
        assert self.buffers
        for name, flat, n in self.buffers:
            assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + n:]).all()), f'{name}: guard overwritten'
            assert not bool(torch.isnan(flat[GUARD:GUARD + n]).any()), f'{name}: elements left unwritten'


@pytest.fixture(scope='module')
def G():
    return R.load_fixture()


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(torch.device('cuda'))


@pytest.fixture(scope='module')
def ref64(G):
    return {n: R.pipeline(R.case_setup(G[n], torch.float64), G[n]['clips'], G[n]['trims']) for n in CASES}


@pytest.mark.parametrize('name', CASES)
def test_cases(G, ref64, be, name):
    g = Guarded(be)
    out = E.run_case(G[name], g, 'cuda')
    g.check()
    n = 7 if G[name]['hinges'] else 6
    assert g.launches[-n:] == [m for m in METHODS if m != 'retarget_hinge' or G[name]['hinges']]      # a constant number of launches
    assert all(o[k].is_cuda for o in out for k in OUTPUTS)
    check_outputs(out, ref64[name], G[name])


def test_batching_is_bitwise(G, be):
    """One call for the three cmu clips (2, 18, 40 -> 28 frames) = three single-clip calls = the same call in another order = a
    second run: no stencil, pairing or reduction crosses a clip boundary."""
    g = G['cmu']
    together, again = E.run_case(g, be, 'cuda'), E.run_case(g, be, 'cuda')
    order = [2, 0, 1]
    shuffled = E.run_case(g, be, 'cuda', order=order)
    n = 0
    for c in range(3):
        alone = E.run_case(g, be, 'cuda', clips=[g['clips'][c]], trims=[g['trims'][c]])[0]
        for k in OUTPUTS:
            n += EM.bits_equal(together[c][k], alone[k])
            EM.bits_equal(together[c][k], shuffled[order.index(c)][k])
            assert torch.equal(together[c][k], again[c][k])
    assert n == (2 + 18 + 28) * 15 * (4 + 3 + 3) + (2 + 18 + 28) * 3


def test_identity_retarget_returns_the_clip(be):
    """amp_humanoid_run.npy onto its own tree: identity mapping, zero-pose T-poses of that tree, identity rotation, scale 1, no
    hinges.  Local rotations come back (normalised) within ulp_f32 + 1e-12 up to sign, the root translation within the same bound once the
    grounding shift - minus the clip's lowest global z, taken here by the emulator's f64 forward kinematics - is added."""
    c = read_clip(RUN_ARGS[0])
    pose = RT.zero_pose(c['node_names'], c['parent_indices'], c['local_translation'])
    g = Guarded(be)
    r = RT.Retargeter(g, 'cuda', pose, pose, {n: n for n in c['node_names']}, [0.0, 0.0, 0.0, 1.0], 1.0, hinges=None)
    out = r.retarget([c])[0]
    g.check()
    rot, root = torch.from_numpy(c['rotation']), torch.from_numpy(c['root_translation'])
    rot = rot / rot.norm(p=2, dim=-1, keepdim=True)          # the file holds 5-decimal quaternions; the retargeter returns unit ones
    got = out['rotation'].cpu().double()
    err = torch.minimum((got - rot).abs().amax(-1), (got + rot).abs().amax(-1))
    assert bool((err <= (EM.ulp_f32(rot).amax(-1) + 1e-12)).all()), float(err.max())
    one = lambda *x: torch.tensor(x, dtype=torch.int32)
    low = E.EmuRetarget().retarget_ground(rot, root, torch.from_numpy(c['local_translation']), torch.from_numpy(RT.tree_table(c['parent_indices'])),
                                          one(0), one(rot.shape[0]))
    want = root.clone()
    want[:, 2] = want[:, 2] + -low[0]
    err = (out['root_translation'].cpu().double() - want).abs()
    assert bool((err <= EM.ulp_f32(want) + 1e-12).all()), float(err.max())
    assert bool(torch.isfinite(out['global_velocity']).all()) and bool(torch.isfinite(out['global_angular_velocity']).all())


def test_config_to_motion_library_end_to_end(G, be, tmp_path):
    """Retargeter.from_config on the fixture's copies of the reference's files -> write_clip -> DeviceMotionLib.from_file ->
    get_motion_state at 50 seeded times = the from_clips route, which never touches the disk."""
    r = RT.Retargeter.from_config(os.path.join(R.RETARGET_DIR, 'retarget_sfu_to_amp.json'), R.RETARGET_DIR, be, 'cuda')
    clips = r.retarget([dict(c, rotation=c['rotation'].numpy(), root_translation=c['root_translation'].numpy()) for c in G['sfu']['clips']])
    path = str(tmp_path / 'sfu_17.npy')
    write_clip(path, clips[1])
    a = DeviceMotionLib.from_file(path, *RUN_ARGS[1:], be, 'cuda')
    b = DeviceMotionLib.from_clips(clips[1:], *RUN_ARGS[1:], be, 'cuda')
    for k in EM.ARRAYS + EM.TABLES:
        assert torch.equal(a.clips[k], b.clips[k]), k
    gen = torch.Generator().manual_seed(5)
    ids = torch.zeros(50, dtype=torch.int64, device='cuda')
    times = (torch.rand(50, generator=gen) * float(a.get_motion_length(ids[:1])[0])).cuda()
    for x, y in zip(a.get_motion_state(ids, times), b.get_motion_state(ids, times)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    both = DeviceMotionLib.from_clips(clips, *RUN_ARGS[1:], be, 'cuda', weights=[1.0, 3.0])
    assert both.num_motions() == 2 and both.clips['num_frames'].tolist() == [3, 17]


def test_operators_equal_the_backend_methods(G, be):
    import ase_amd.ops  # noqa: F401
    ops = torch.ops.ase_hip
    g = G['cmu']
    src, tgt = R.case_poses(g)
    r = RT.Retargeter(be, 'cuda', src, tgt, g['joint_mapping'], g['rotation'], g['scale'], root_height_offset=g['root_height_offset'])
    rot = torch.cat([c['rotation'] for c in g['clips']]).double().cuda()
    root = torch.cat([c['root_translation'] for c in g['clips']]).double().cuda()
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device='cuda')
    first, num, src_first = i32([0, 2, 20]), i32([2, 18, 28]), i32([0, 2, 25])
    frame_clip = torch.repeat_interleave(torch.arange(3, dtype=torch.int32), torch.tensor([2, 18, 28])).cuda()
    fps = torch.tensor([120.0, 60.0, 30.0], dtype=torch.float64, device='cuda')
    t, maps = r.tabs, (first, num, src_first, frame_clip)

    def same(a, b):
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            EM.bits_equal(x, y)
        return a
    gs = same(ops.retarget_fk(rot, 0, r.src_tree, *maps), be.retarget_fk(rot, 0, r.src_tree, *maps))
    args = (gs, t['rs_body'], t['rs_parent'], t['rt_src'], t['rt_tree'], r.params)
    gc = same(ops.retarget_chain(*args), be.retarget_chain(*args))
    args = (gc, r.tpose_global, r.target_global, root, r.params, t['rt_body'], t['ancestor'], r.tgt_parent, *maps)
    lr, rt = same(tuple(ops.retarget_pose(*args)), be.retarget_pose(*args))
    args = (lr, rt, r.tgt_offsets, r.tgt_tree, r.roles)
    lr = same(ops.retarget_hinge(*args), be.retarget_hinge(*args))
    args = (lr, rt, r.tgt_offsets, r.tgt_tree, first, num)
    low = same(ops.retarget_ground(*args), be.retarget_ground(*args))
    args = (lr, rt, low, r.params, r.tgt_offsets, r.tgt_tree, frame_clip)
    gr, gt, _, _ = same(tuple(ops.retarget_finish(*args)), be.retarget_finish(*args))
    args = (gr, gt, first, num, fps, frame_clip)
    vel, _ = same(tuple(ops.retarget_velocity(*args)), be.retarget_velocity(*args))
    whole = r.retarget([dict(c, rotation=c['rotation'].numpy(), root_translation=c['root_translation'].numpy()) for c in g['clips']],
                       trim=[tuple(x) for x in g['trims']])
    EM.bits_equal(vel, torch.cat([w['global_velocity'] for w in whole]))
    with pytest.raises(RuntimeError, match='retarget_fk'):
        ops.retarget_fk(rot.float(), 0, r.src_tree, *maps)


def test_refusals_leave_the_outputs_alone(be):
    nan = lambda *shape, dt=torch.float64: torch.full(shape, float('nan'), dtype=dt, device='cuda')
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device='cuda')
    rot, tree = torch.zeros(2, 2, 4, dtype=torch.float64, device='cuda'), i32([[0, 0, -1], [1, 0, 1]])
    out = nan(2, 2, 4)
    with pytest.raises(L.AseHipError, match='mode 5'):
        be.retarget_fk(rot, 5, tree, i32([0]), i32([2]), i32([0]), i32([0, 0]), out=out)
    vel, ang = nan(1, 2, 3, dt=torch.float32), nan(1, 2, 3, dt=torch.float32)
    with pytest.raises(L.AseHipError, match='a clip has 2 or more'):
        be.retarget_velocity(rot[:1], torch.zeros(1, 2, 3, dtype=torch.float64, device='cuda'), i32([0]), i32([1]),
                             torch.ones(1, dtype=torch.float64, device='cuda'), i32([0]), out=(vel, ang))
    # tables that do not describe the frames (a row of no clip, a chain that leaves the tree): the items write nothing
    be.retarget_fk(rot, 0, i32([[0, 0, -1], [1, 0, 7]]), i32([0]), i32([1]), i32([0]), i32([0, -1]), out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isnan(out[0, 1]).all()) and not bool(torch.isnan(out[0, 0]).any())
    assert bool(torch.isnan(vel).all()) and bool(torch.isnan(ang).all())
