"""What the GPU tests of the device-side start-up and evaluation stages share: inputs onto the device, results compared bit for bit."""
import numpy as np
import torch

DEV = "cuda:0"


def t(a, dtype=None):
    """A tensor or array on the device, contiguous, converted to dtype when one is given."""
    a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (a if dtype is None else a.to(dtype)).to(DEV).contiguous()


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits_equal(got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)
