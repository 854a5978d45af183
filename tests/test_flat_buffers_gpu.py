"""GPU: the net's flat buffers (parameters, gradients, optimizer history) hold finite values from allocation on, whatever the device
allocator hands out.  The slices of the edges are 128-float aligned and nobody writes the padding between them, so after tensors of
bytes or integers have been freed (0xFF bytes read as float are a NaN) the padding used to keep their bit patterns: a whole-buffer check
such as ``np.isfinite(net.parameters_.ToNumpy()).all()`` then failed although every parameter was fine."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_flat_buffers_are_finite_after_the_allocator_held_nan_patterns():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    from test_net_gpu import build, small_alexnet
    Matrix.SetupCUDADevice(0)
    blocks = [torch.full((n,), 255, dtype=torch.uint8, device="cuda") for n in (4096, 65536, 262144, 1 << 20, 4 << 20) for _ in range(8)]
    torch.cuda.synchronize()
    del blocks                                        # freed blocks stay with the caching allocator, contents and all
    net = build(small_alexnet(), 8, fused=True)
    padded = net.parameters_.GetNumEls() - net.NumParameters()
    assert padded > 0                                 # there is padding to speak of
    for m in (net.parameters_, net.grad_parameters_, net.history_):
        assert np.isfinite(m.ToNumpy()).all()
    net.TrainOneBatch()
    for m in (net.parameters_, net.grad_parameters_, net.history_):
        assert np.isfinite(m.ToNumpy()).all()
