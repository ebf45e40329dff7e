"""The float64 model of the present pass (tests/present_model.py) against the oracle and the reference's own frames, and the
conditions that make the table's images worth running on the GPU (tests/test_present_paths_gpu.py).  All on the CPU.

Measured here — the float32 restatement's own error: the oracle (oracle/denoise_oracle.c) lies within ORACLE_TO_MODEL of
the float64 model on every finite pixel of every case of the table, the largest on `MODEL_WORST_CASE`; against the three
tests/golden/ref/present_*.npz frames of the reference's shader the model is inside the same 1e-4 the oracle is held to.
The GPU tolerance is the project's 1e-4 and does not derive from this figure.
"""
import numpy as np
import pytest

from tests import present_model as M

TOL = 1e-4            # the pass's tolerance per channel (north_star)
SENSITIVE = 2e-4      # a misplaced tap or a wrong addressing mode must move some channel of some pixel by more than this
# the largest oracle-to-model distance over the table, measured by test_model_agrees_with_the_oracle_on_every_case (it prints every
# case's figure before it asserts): the float32 restatement's own rounding, summed over up to 258 taps
ORACLE_TO_MODEL = 1.2e-6
MODEL_WORST_CASE = "table_global_s256"

model_of = M.reference_of


def _distance(a, b):
    """Largest channel difference over the pixels finite in both, and whether the NaN patterns are equal."""
    na, nb = np.isnan(a).any(axis=2), np.isnan(b).any(axis=2)
    both = ~na & ~nb
    return (float(np.abs(a[both] - b[both]).max()) if both.any() else 0.0), bool(np.array_equal(na, nb))


def _differs(a, b):
    """Per pixel: some channel moved by more than SENSITIVE, or the pixel is NaN in one frame alone."""
    na, nb = np.isnan(a).any(axis=2), np.isnan(b).any(axis=2)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b).max(axis=2)
    return np.where(na | nb, na != nb, d > SENSITIVE)


# ------------------------------------------------------------------------------------------------- model against oracle
@pytest.mark.parametrize("case", M.CASES, ids=M.CASE_IDS)
def test_model_agrees_with_the_oracle_on_every_case(case):
    img, m, fo, uo = model_of(case)
    got = m.rgb()
    d, same_nan = _distance(got, fo[..., :3].astype(np.float64))
    print(f"{case.id}: oracle to model {d:.3e}, finite pixels {int((~np.isnan(got).any(axis=2)).sum())} of {got.shape[0] * got.shape[1]}")
    assert same_nan, "NaN where the shader has NaN: the model and the oracle disagree on which pixels"
    assert d <= TOL, "the oracle alone must be inside the tolerance of the model: change this case's image, never the tolerance"
    assert d <= ORACLE_TO_MODEL, "ORACLE_TO_MODEL is the measured maximum: re-measure and state it"
    mu = M.unorm8(got)
    assert np.abs(mu.astype(int) - uo[..., :3].astype(int)).max() <= 1
    assert (mu[np.isnan(got)] == 0).all()
    if case.id not in M.INSENSITIVE:
        assert (~np.isnan(got)).any()
    if case.samples == 0:
        assert np.isnan(got).all() and np.isnan(fo[..., :3]).all()   # 0.5 / 0 * pow(0, bias): the shader's own division by zero
    if case.family == "black":
        nan = np.isnan(got).any(axis=2)
        assert 8 <= nan.sum() < nan.size // 2, "the black texels must poison some pixels and leave most"


def test_model_worst_case_is_the_one_stated():
    worst = max(M.CASES, key=lambda c: _distance(model_of(c)[1].rgb(), model_of(c)[2][..., :3].astype(np.float64))[0])
    d = _distance(model_of(worst)[1].rgb(), model_of(worst)[2][..., :3].astype(np.float64))[0]
    assert worst.id == MODEL_WORST_CASE and 0.5 * ORACLE_TO_MODEL <= d <= ORACLE_TO_MODEL, (worst.id, d)


def test_model_agrees_with_the_reference_shaders_frames():
    """tests/golden/ref/present_*.npz: frames of image.vert + image.frag themselves, under test_ref_gl's own rule."""
    from tests.test_ref_gl import PRESENT, _compare_present, _present_args
    assert len(PRESENT) >= 3
    for path in PRESENT:
        z = np.load(path)
        ow, oh = (int(v) for v in z["out_size"])
        m = M.PresentModel(z["image_rgba8"], ow, oh, keep_taps=False, **_present_args(z))
        _compare_present(m.rgb().astype(np.float32), z)


def test_model_fixed_point_and_perturbations_on_a_constant_image():
    img = np.zeros((9, 11, 4), dtype=np.uint8)
    img[...] = (200, 120, 40, 255)
    m = M.PresentModel(img, 13, 7)
    want = np.array([200, 120, 40]) / 255.0
    assert np.abs(m.rgb() - want).max() < 1e-12
    assert np.abs(m.shifted(3, 1, 0) - want).max() < 1e-12
    assert np.abs(M.PresentModel(img, 13, 7, clamp=True).rgb() - want).max() < 1e-12


# --------------------------------------------------------------------------------------------------------- sensitivity
def _bands(case):
    """The output pixels whose taps reach over the left, right, top and bottom edge of the image."""
    W, H = case.size
    reach = float(M.launcher_terms(W, H, case.out[0], case.out[1], case.samples, case.pixel_multiplier)[0]) - 2.0
    oy, ox = np.mgrid[0:case.out[1], 0:case.out[0]]
    s, t = (ox + 0.5) / case.out[0] * W - 0.5, (oy + 0.5) / case.out[1] * H - 0.5
    return {"left": s < reach, "right": s > W - 1 - reach, "top": t < reach, "bottom": t > H - 1 - reach}


@pytest.mark.parametrize("case", [c for c in M.CASES if c.id not in M.INSENSITIVE], ids=lambda c: c.id)
def test_every_single_misplaced_tap_moves_the_models_output(case):
    img, m, _, _ = model_of(case)
    base = m.rgb()
    moves = ((1, 0),) if case.id in M.X_ONLY else ((1, 0), (0, 1))
    for k in range(case.samples + 1):
        for dx, dy in moves:
            assert _differs(base, m.shifted(k, dx, dy)).any(), f"sample {k} read ({dx}, {dy}) texels off goes unseen on this image"


@pytest.mark.parametrize("case", [c for c in M.CASES if c.id not in M.INSENSITIVE], ids=lambda c: c.id)
def test_clamp_instead_of_repeat_moves_the_models_output_in_every_border_band(case):
    img, m, _, _ = model_of(case)
    moved = _differs(m.rgb(), M.PresentModel(img, case.out[0], case.out[1], clamp=True, keep_taps=False, **case.params()).rgb())
    if case.id in M.NO_BORDER:
        assert not moved.any() and not any(b.any() for b in _bands(case).values())
        return
    for name, band in _bands(case).items():
        if case.id in M.X_ONLY and name in ("top", "bottom"):
            continue
        assert (moved & band).any(), f"clamp-to-edge goes unseen in the {name} band"
    assert not (moved & ~np.logical_or.reduce(list(_bands(case).values()))).any(), "addressing matters only where taps cross an edge"


def test_the_insensitive_cases_are_the_ones_that_cannot_be_sensitive():
    for cid in M.INSENSITIVE:
        c = M.BY_ID[cid]
        assert c.size == (1, 1) or c.samples == 0
    for cid in M.X_ONLY:
        assert M.BY_ID[cid].size[1] == 1 and M.BY_ID[cid].size[0] > 1
    assert not [c.id for c in M.CASES if (c.size == (1, 1) or c.samples == 0) and c.id not in M.INSENSITIVE]


# ------------------------------------------------------------------------------------------------------ the launcher's rule
def test_the_table_reaches_all_four_kernels_and_both_sides_of_every_boundary():
    """kernel_for restates launch_denoise's selection (zig_vulkan_amd/csrc/vrt_post.hip).  When that rule changes, this test, kernel_for
    and the table have to be revisited: the cases sit a hair on either side of today's boundaries."""
    for c in M.CASES:
        assert c.kernel is not None and c.picked() == c.kernel, (c.id, c.picked())
    assert {c.kernel for c in M.CASES} == {M.TILE20, M.TILE0, M.NEAR, M.GENERAL}
    for what, a, b in M.BOUNDARIES:
        ca, cb = M.BY_ID[a], M.BY_ID[b]
        assert ca.picked() != cb.picked(), what
        differing = [k for k in ("size", "out", "samples", "distribution_bias", "pixel_multiplier", "inverse_hue_tolerance", "family") if getattr(ca, k) != getattr(cb, k)]
        if ca.out == ca.size and cb.out == cb.size and "size" in differing:   # (an output 1 : 1 follows the image)
            differing.remove("out")
        assert len(differing) == 1, (what, differing)
    # how close to the boundaries: the staged kernel's box at no less than 31.9 of its 32 texels, the near wrap within 0.05 texel of the image
    for cid in ("bound_64x64_tol20_m2.68", "bound_80x72_tol7_m2.68", "scale_down_x_at_bound"):
        c = M.BY_ID[cid]
        _, sx, sy = M.launcher_terms(*c.size, *c.out, c.samples, c.pixel_multiplier)
        assert 31.9 <= max(sx, sy) <= 32.0
    c = M.BY_ID["scale_down_y_alone_past_bound"]
    _, sx, sy = M.launcher_terms(*c.size, *c.out, c.samples, c.pixel_multiplier)
    assert sx <= 32.0 < sy
    for cid, lo, hi in (("wrap_24x16_m4.1", 15.95, 16.0), ("wrap_24x16_m4.12", 16.0, 16.05), ("wrap_24x16_m-4.1", 15.95, 16.0), ("wrap_24x16_m-4.12", 16.0, 16.05)):
        c = M.BY_ID[cid]
        assert lo <= float(M.launcher_terms(*c.size, *c.out, c.samples, c.pixel_multiplier)[0]) <= hi
    # the table: exactly full by thread k < n (samples 255 -> n = 256), and the first samples past it
    assert {254, 255} <= {c.samples for c in M.CASES if c.kernel in (M.TILE20, M.TILE0)}
    assert {255, 256, 257} <= {c.samples for c in M.CASES if c.kernel == M.NEAR}
    assert {0, 1} <= {c.samples for c in M.CASES}
