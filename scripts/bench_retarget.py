"""Wall time of one ``Retargeter.retarget`` call on the GPU: 64 copies of the 40-frame cmu clip of
tests/golden/retarget.pt, and 64 clips of 300 frames (that clip played forth and back).  Eager calls, 5 warm-ups, 20 timed calls
between device synchronisations; the launch count is the backend calls of one ``retarget``.  Appends JSON lines to --out
(default profiles/retarget.jsonl).  The reference pipeline's CPU time for the same clips is taken by
scripts/make_golden_retarget.py --time, on another machine: the two figures are not comparable as a ratio.

    python scripts/bench_retarget.py [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ase_amd import retarget as RT                   # noqa: E402
from ase_amd.backend import HipBackend               # noqa: E402
from tests import ref_retarget as R                  # noqa: E402


class Counting:
    def __init__(self, be):
        self.be, self.n = be, 0

    def __getattr__(self, name):
        fn = getattr(self.be, name)
        if not name.startswith('retarget_'):
            return fn

        def call(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'retarget.jsonl'))
    args = ap.parse_args()
    g = R.load_fixture()['cmu']
    src, tgt = R.case_poses(g)
    be = Counting(HipBackend(torch.device('cuda')))
    r = RT.Retargeter(be, 'cuda', src, tgt, g['joint_mapping'], g['rotation'], g['scale'], root_height_offset=g['root_height_offset'])
    clip = g['clips'][2]
    forth_back = lambda x: torch.cat([x, x.flip(0)] * 4)[:300]
    sets = {'64 x 40 frames': [dict(clip, rotation=clip['rotation'].cuda(), root_translation=clip['root_translation'].cuda())] * 64,
            '64 x 300 frames': [dict(clip, rotation=forth_back(clip['rotation']).cuda(),
                                     root_translation=forth_back(clip['root_translation']).cuda())] * 64}
    rows = []
    for label, clips in sets.items():
        for _ in range(5):
            r.retarget(clips)
        torch.cuda.synchronize()
        be.n = 0
        t0 = time.perf_counter()
        for _ in range(20):
            r.retarget(clips)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 20
        rows.append({'what': 'Retargeter.retarget, eager, source clips resident on the device', 'gpu': torch.cuda.get_device_name(0),
                     'clips': label, 'ms_per_call': round(dt * 1e3, 3), 'launches_per_call': be.n // 20})
        print(json.dumps(rows[-1]))
    with open(args.out, 'a') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
