"""The present pass's four kernels at the conditions that choose between them (launch_denoise, zig_vulkan_amd/csrc/vrt_post.hip).

Every case of tests/present_model.py's table puts a synthetic image — one on which a single misplaced tap, or clamp instead of
repeat, moves the result by more than twice the tolerance (tests/test_present_model.py proves that on the CPU) — behind the
context's target and compares vrt_denoise with the oracle as tests/test_denoise.py does (NaN pattern equal, float within 1e-4,
RGBA8 within 1 LSB, alpha 255) and with the float64 model (within 1e-4 where both are finite).  Which kernel a case takes is
asserted by the CPU test of the launcher's rule, never on the device.
"""
import numpy as np
import pytest

from tests import present_model as M

TOL = 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("case", M.CASES, ids=M.CASE_IDS)
def test_hip_denoise_matches_oracle_and_model_at_the_launchers_boundaries(case):
    import torch
    from zig_vulkan_amd import BrickGrid, Config, VoxelRT
    img, model, fo, uo = M.reference_of(case)
    w, h = case.size
    dev = torch.from_numpy(np.ascontiguousarray(img).reshape(-1).copy()).cuda()
    rt = VoxelRT(BrickGrid(1, 1, 1), Config(internal_resolution_width=w, internal_resolution_height=h, external_target_rgba8=dev.data_ptr()))
    try:
        u, f = rt.denoise(case.out[0], case.out[1], want_float=True, **case.params())
    finally:
        rt.deinit()
    assert f.shape == fo.shape and u.shape == uo.shape
    nan_o, nan_k = np.isnan(fo[..., :3]).any(axis=-1), np.isnan(f[..., :3]).any(axis=-1)
    ok = ~nan_o
    mf = model.rgb()
    finite = ok & ~nan_k & ~np.isnan(mf).any(axis=-1)
    d_oracle = float(np.abs(f[ok & ~nan_k] - fo[ok & ~nan_k]).max()) if (ok & ~nan_k).any() else 0.0
    d_model = float(np.abs(f[..., :3][finite] - mf[finite]).max()) if finite.any() else 0.0
    print(f"{case.id} ({case.kernel}): to oracle {d_oracle:.3e}, to model {d_model:.3e}, NaN pixels {int(nan_k.sum())} / oracle {int(nan_o.sum())}")
    assert np.array_equal(nan_o, nan_k), "NaN where the shader has NaN, and nowhere else"
    assert np.array_equal(np.isnan(fo[..., :3]), np.isnan(f[..., :3]))
    assert d_oracle <= TOL
    assert np.array_equal(np.isnan(mf).any(axis=-1), nan_k) and d_model <= TOL
    assert np.abs(u.astype(int) - uo.astype(int)).max() <= 1
    assert (u[..., 3] == 255).all() and (f[..., 3] == 1.0).all()
    assert (u[..., :3][nan_k] == 0).all()           # the UNORM store of a NaN
    if case.samples > 0:
        assert ok.any()
    else:
        assert nan_k.all()
