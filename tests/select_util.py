"""What the GPU tests of the streamed selection share (op level: tcar_select_*; engine level: the serve steps): the skip without a
GPU, the comparison within the project's logits gate, the loaded library as a fixture and a pointer into a tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

RTOL = 1e-3


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def close(got, want, rtol=RTOL, atol_scale=2e-5, name=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = np.abs(got - want)
    bad = err > rtol * np.abs(want) + atol_scale * scale + 1e-9
    assert not bad.any(), "%s: %d/%d off, max err %.3e (scale %.3e)" % (name, bad.sum(), bad.size, err.max(), scale)


@pytest.fixture(scope="module")
def lib():
    _need_gpu()
    from tcar_amd import _lib
    return _lib.load()


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)
