"""Golden hyper-parameter tables: the layer widths / activations and the scalar config entries of the reference's three
training yaml files, as the yaml loader returns them (numeric strings such as '2e-5' kept as strings, so that the test
still exercises ase_amd.cfg.normalize).     python oracle/make_golden_cfg.py -> tests/golden/reference_cfg.json"""
import json
import os

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = '/root/reference/ase/data/cfg/train/rlg'
FILES = {'ase': 'ase_humanoid.yaml', 'amp': 'amp_humanoid.yaml', 'hrl': 'hrl_humanoid.yaml'}


def main():
    out = {}
    for kind, fn in FILES.items():
        ref = yaml.safe_load(open(os.path.join(REF_DIR, fn)))['params']
        net = {part: {'units': ref['network'][part]['units'], 'activation': ref['network'][part]['activation']}
               for part in ('mlp', 'disc', 'enc') if part in ref['network']}
        conf = {k: v for k, v in ref['config'].items() if isinstance(v, (int, float, bool, str))}
        out[kind] = {'file': fn, 'network': net, 'config': conf}
    path = os.path.join(HERE, '..', 'tests', 'golden', 'reference_cfg.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', os.path.normpath(path))


if __name__ == '__main__':
    main()
