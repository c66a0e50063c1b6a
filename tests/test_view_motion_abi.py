"""The host checks of ``ase_hip_motion_sync``: every refusal, without a launch and without a GPU, and the
binding's arity."""
import ctypes

from ase_amd import lib as L

LAST = b'body strides do not cover'        # the message of the entry's last check


def _entry_args(**kw):
    """SYNC arguments that pass every check of the entry BUT THE LAST: ba_sb = 2 is below a body's three floats, so no call built
    here can reach the launch, whatever else it carries and whichever earlier check it is meant to show."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    offs, bodies = (ctypes.c_int32 * 3)(0, 3, 4), (ctypes.c_int32 * 2)(1, 2)
    a = dict(mode=L.MOTION_SYNC, gts=p, grs=p, lrs=p, n_bodies=3, lengths=p, num_frames=p, dt=p, length_starts=p, num_motions=2,
             dof_body_ids=bodies, dof_offsets=offs, n_joints=2, motion_ids=p, progress_buf=p, motion_dt=1.0 / 30.0, reset_buf=p,
             terminate_buf=p, root_states=p, ld_root=13, dof_pos=p, dp_se=8, dp_sd=2, dof_vel=p, dv_se=8, dv_sd=2, body_pos=p, bp_se=9,
             bp_sb=3, body_rot=p, br_se=12, br_sb=4, body_vel=p, bv_se=9, bv_sb=3, body_ang_vel=p, ba_se=9, ba_sb=2, env_ids=None, n_ids=0,
             ids_out=None, n_envs=4, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    assert a['mode'] != L.MOTION_SYNC or (a['body_ang_vel'] is not None and a['ba_sb'] < 3), 'every SYNC call keeps the defect of the last check'
    return list(a.values()), (buf, offs, bodies), p


def _refusal(lib, **kw):
    args, keep, _ = _entry_args(**kw)
    rc = lib.ase_hip_motion_sync(*args)
    msg = lib.ase_hip_last_error()
    assert rc == -1 and msg.startswith(b'motion_sync:'), (kw, rc, msg)
    return msg


def test_binding():
    lib = L.load()
    assert L.ABI_VERSION == 9 and lib.ase_hip_abi_version() == 9 and len(L.SIGNATURES['ase_hip_motion_sync']) == 43
    assert (L.MOTION_SYNC, L.MOTION_RESET, L.MOTION_SYNC_MAX_BODIES) == (0, 1, 64)


def test_every_refusal_of_the_entry_without_a_launch():
    lib = L.load()
    _, _, p = _entry_args()
    bad_first = (ctypes.c_int32 * 3)(1, 3, 4)
    two_dofs = (ctypes.c_int32 * 3)(0, 2, 4)
    far_body = (ctypes.c_int32 * 2)(1, 3)
    neg_body = (ctypes.c_int32 * 2)(-1, 2)
    defects = [
        (dict(mode=2), b'mode 2'),
        (dict(mode=-1), b'mode -1'),
        (dict(n_envs=0), b'bad size'),
        (dict(num_motions=0), b'num_motions 0 below 1'),
        (dict(motion_ids=None), b'needs motion_ids'),
        (dict(progress_buf=None), b'needs motion_ids'),
        (dict(reset_buf=None), b'needs motion_ids'),
        (dict(terminate_buf=None), b'needs motion_ids'),
        (dict(env_ids=p, n_ids=1), b'runs on every environment'),
        (dict(ids_out=p), b'runs on every environment'),
        (dict(n_ids=2), b'runs on every environment'),
        (dict(gts=None), b'null clip operand'),
        (dict(grs=None), b'null clip operand'),
        (dict(lrs=None), b'null clip operand'),
        (dict(lengths=None), b'null clip operand'),
        (dict(length_starts=None), b'null clip operand'),
        (dict(dof_offsets=None), b'null clip operand'),
        (dict(root_states=None), b'needs root_states'),
        (dict(dof_pos=None), b'needs root_states'),
        (dict(dof_vel=None), b'needs root_states'),
        (dict(n_bodies=0), b'bad sizes'),
        (dict(n_bodies=65), b'bad sizes'),
        (dict(n_joints=0), b'bad sizes'),
        (dict(n_joints=33), b'bad sizes'),
        (dict(dof_offsets=bad_first), b'first offset 1'),
        (dict(dof_offsets=two_dofs), b'joint 0: 2 dofs'),
        (dict(dof_body_ids=far_body), b'joint 1: 1 dofs on body 3'),
        (dict(dof_body_ids=neg_body), b'joint 0: 3 dofs on body -1'),
        (dict(ld_root=12), b'root_states row stride 12 below 13'),
        (dict(dp_sd=0), b'dof_pos / dof_vel strides'),
        (dict(dv_sd=0), b'dof_pos / dof_vel strides'),
        (dict(dp_se=6), b'dof_pos / dof_vel strides'),
        (dict(dv_se=6), b'dof_pos / dof_vel strides'),
        (dict(dp_sd=1, dp_se=3), b'dof_pos / dof_vel strides'),
        # RESET: the refusals of its own operand pattern
        (dict(mode=L.MOTION_RESET, n_ids=3), b'n_ids 3 without env_ids'),
        (dict(mode=L.MOTION_RESET, env_ids=p, n_ids=-1), b'n_ids -1 with env_ids'),
        (dict(mode=L.MOTION_RESET, env_ids=p, n_ids=5), b'n_ids 5 with env_ids'),
        (dict(mode=L.MOTION_RESET, env_ids=p, n_ids=2, ids_out=p), b'ids_out is the export'),
        (dict(mode=L.MOTION_RESET), b'writes no state'),
        (dict(mode=L.MOTION_RESET, root_states=None, dof_pos=None, dof_vel=None, body_pos=None, body_rot=None, body_vel=None),
         b'writes no state'),
    ]
    for kw, text in defects:
        msg = _refusal(lib, **kw)
        assert text in msg and LAST not in msg, (kw, msg)

    def passes(**kw):
        msg = _refusal(lib, **kw)
        assert LAST in msg, (kw, msg)
    # the good side of every check: the values at its edge reach the last check
    passes()
    passes(n_envs=1)
    passes(num_motions=1)
    passes(n_bodies=64, bp_se=192, br_se=256, bv_se=192, ba_se=192)
    passes(ld_root=13)
    passes(ld_root=1 << 40)
    passes(dp_se=7, dv_se=7)                       # (D - 1) * 2 + 1
    passes(dp_sd=1, dp_se=4, dv_sd=1, dv_se=4)
    passes(body_pos=None, body_rot=None, body_vel=None)
    passes(motion_dt=0.0)
    # the last check's own cases
    for kw in (dict(bp_sb=2), dict(bp_se=8), dict(br_sb=3), dict(br_se=11), dict(bv_sb=2), dict(bv_se=8), dict(ba_se=8), dict(ba_sb=-3)):
        passes(**kw)


def test_reset_with_an_empty_list_is_a_no_op():
    """An id list of length 0 resets nothing: the entry returns before any launch."""
    lib = L.load()
    nothing = dict(root_states=None, dof_pos=None, dof_vel=None, body_pos=None, body_rot=None, body_vel=None, body_ang_vel=None)
    args, keep, p = _entry_args(mode=L.MOTION_RESET, **nothing)
    args[38], args[39] = p, 0
    assert lib.ase_hip_motion_sync(*args) == 0
