"""Time of one view-motion SYNC step on the GPU: ``ViewMotionEnv.motion_sync`` at 4096 environments on a
``ClipPhysics`` (17 bodies, the five-clip library of tests/golden/view_motion.pt), the one launch of ``ase_hip_motion_sync``
against the ``fused=False`` composition - ``motion_state`` once for root, dofs and body positions, once more per further body for
its rotation, and the torch glue - which is made only of entries that existed before the launch: the parent-side yardstick.

HIP events around 100 back-to-back calls, 20 warm-up calls, the forms alternated in one process over seven repeats; median and
range.  The fused step is also timed replayed from a launch program.  The composition holds torch ops and allocations, which a
launch program does not record: it has no recorded form.  Appends one JSON line to --out (default profiles/view_motion.jsonl).

    python scripts/bench_view_motion.py [--out FILE] [--envs N]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ase_amd.backend import HipBackend               # noqa: E402
from tests import emu_view_motion as E               # noqa: E402
from tests import ref_view_motion as RV              # noqa: E402

CALLS, WARMUP, REPEATS = 100, 20, 7


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'view_motion.jsonl'))
    ap.add_argument('--envs', type=int, default=4096)
    args = ap.parse_args()
    be = HipBackend(torch.device('cuda:0'))
    clips = RV.load_fixture()['clips']
    envs = {fused: E.make_env(be, 'cuda:0', clips, args.envs, fused) for fused in (True, False)}
    for env in envs.values():
        env.reset()
        env.progress_buf.copy_(torch.arange(args.envs, device='cuda:0') % 7)      # inside and past the short clips
    prog = be.prog_create()
    be.prog_begin(prog)
    envs[True].motion_sync()
    be.prog_end(prog)
    forms = {'fused eager': envs[True].motion_sync, 'fused recorded': lambda: be.prog_launch(prog), 'composition eager': envs[False].motion_sync}
    try:
        for fn in forms.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in forms}
        for _ in range(REPEATS):
            for k, fn in forms.items():
                samples[k].append(timed(fn))
        launches = be.prog_size(prog)
    finally:
        be.prog_destroy(prog)
    same = all(torch.equal(getattr(envs[True].physics, k), getattr(envs[False].physics, k)) for k in ('root_states', 'dof_state', 'rigid_body_state'))
    row = {'what': 'ViewMotionEnv.motion_sync on ClipPhysics: one SYNC step', 'gpu': torch.cuda.get_device_name(0), 'envs': args.envs,
           'bodies': RV.BODIES, 'calls': CALLS, 'repeats': REPEATS, 'fused_launches': launches, 'composition_motion_state_calls': RV.BODIES,
           'fused_equals_composition_bitwise': same,
           'us_per_call': {k: {'median': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}
                           for k, v in samples.items()}}
    print(json.dumps(row))
    with open(args.out, 'a') as f:
        f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
