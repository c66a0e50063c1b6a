"""tests/test_forward_engine_emu.py's comparison through libase_hip.so on the GPU: the forward-only engine and the trainer issue
the same launches on the same operands and no forward launch uses atomics, so the outputs are compared bitwise."""
import os

import pytest
import torch

from tests.test_forward_engine_emu import compare_engines

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', ['ase_tiny', 'amp_tiny'])
def test_forward_engine_equals_update_engine_gpu(name, dtype, golden_dir):
    from ase_amd.backend import HipBackend
    G = torch.load(os.path.join(golden_dir, name + '.pt'), weights_only=False)
    compare_engines(G, lambda: HipBackend('cuda:0'), dtype, device='cuda:0')
    torch.cuda.synchronize()


def test_inference_engine_builds_a_forward_engine(golden_dir):
    from ase_amd.engine import UpdateEngine
    from ase_amd.forward import ForwardEngine
    from ase_amd.inference import InferenceEngine
    from tests.helpers import build_net
    G = torch.load(os.path.join(golden_dir, 'ase_tiny.pt'), weights_only=False)
    eng = InferenceEngine(build_net(G, 'cuda:0')).eng
    assert isinstance(eng, ForwardEngine) and not isinstance(eng, UpdateEngine)
