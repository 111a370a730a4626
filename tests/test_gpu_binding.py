"""GPU test (``pytest -m gpu``) of the engine wrappers that no other test calls in its own process: ``profile_enable`` /
``profile_read``, which only bench.py uses.  ``smil_profile_read`` takes two host pointers through ``byref``."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_profile_hook_counts_the_tile_kernel_launches(tables):
    from smilify_amd import engine

    t = tables("synthetic")
    S = 32
    dm = engine.DeviceModel(t, DEV)
    v = torch.from_numpy(np.asarray(t.v_template, np.float32))
    v = (v - v.mean(0)) / float((v - v.mean(0)).norm(dim=1).max())
    cams = engine.CameraSet(torch.eye(3, device=DEV)[None].contiguous(), torch.tensor([[0.0, 0.0, 2.7]], device=DEV),
                            torch.tensor([60.0], device=DEV), None, 1, S)
    ndc, _ = engine.project(cams, v[None].contiguous().to(DEV), want_yx=False)
    engine.profile_enable(True)
    try:
        assert engine.profile_read() == (0.0, 0)
        sil = engine.silhouette_forward(dm, ndc, S)
        ms, n = engine.profile_read()
        assert type(ms) is float and type(n) is int
        assert n == 1 and math.isfinite(ms) and ms > 0.0, (ms, n)
        assert engine.profile_read() == (0.0, 0)  # a read starts the count again
    finally:
        engine.profile_enable(False)
    engine.silhouette_forward(dm, ndc, S)
    assert engine.profile_read() == (0.0, 0)      # switched off: nothing is recorded
    assert sil.shape == (1, S, S) and sil.dtype == torch.float32 and float(sil.max()) > 0.5
