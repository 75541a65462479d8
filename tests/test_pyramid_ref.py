"""CPU tests of the scale pyramid's rules (include/pgx.h, "Scale pyramid"): the library's host helper pgx_pyramid_dims against
the numpy restatement tests/pyramid_ref.py, the argument checks, the source-index bounds rule 3 promises, a constant image
through every level, and the claim the mode exists for -- on the CPU oracle alone, an image and its half-size copy match at
hundreds of keypoints with the pyramid and at next to none without it."""
import numpy as np
import pytest

import photogrammetry_amd as pg
import pyramid_ref as pr
from photogrammetry_amd import _lib

STEPS = [69632, 78643, 92682, 100000, 131071, 131072]
SIZES = [(161, 140), (40, 30), (1920, 1080), (65535, 16)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("step", STEPS)
def test_dims_equal_the_restatement(W, H, step):
    d, s = pg.pyramid_dims(W, H, 8, step)
    ed, es = pr.dims(W, H, 8, step)
    assert d.dtype == np.int32 and s.dtype == np.int32 and d.shape == (8, 2) and s.shape == (8,)
    assert d.tolist() == ed.tolist() and s.tolist() == es.tolist()
    for n in (1, 3):                                         # fewer levels: a prefix
        dn, sn = pg.pyramid_dims(W, H, n, step)
        assert dn.tolist() == ed[:n].tolist() and sn.tolist() == es[:n].tolist()


def test_dims_examples():
    d, s = pg.pyramid_dims(161, 140, 8, 92682)
    assert d.tolist() == [[161, 140], [113, 98], [79, 69], [55, 48], [38, 33], [26, 23], [18, 16], [0, 0]]
    assert s[0] == 65536 and s[1] == 92682 and s[2] == (92682 * 92682 + 32768) >> 16
    d, _ = pg.pyramid_dims(40, 30, 8, 131072)                # 20 x 15: the height falls below 16
    assert d.tolist() == [[40, 30]] + [[0, 0]] * 7
    d, s = pg.pyramid_dims(65535, 16, 8, 69632)              # 16 / 1.0625 = 15.06: empty from level 1, the scale goes on
    assert d.tolist() == [[65535, 16]] + [[0, 0]] * 7 and (np.diff(s) > 0).all()
    assert pg.pyramid_dims(2048, 2048, 8, 131072)[1].tolist() == [65536 << l for l in range(8)]
    assert pg.pyramid_dims(8, 8, 2, 131072)[0].tolist() == [[8, 8], [0, 0]]   # level 0 is the frame whatever its size


def test_bad_arguments():
    L = _lib.lib()
    d, s = np.zeros((8, 2), np.int32), np.zeros(8, np.int32)
    for n, step in [(0, 92682), (9, 92682), (-1, 92682), (4, 69631), (4, 131073), (4, 0), (4, -92682)]:
        assert L.pgx_pyramid_dims(161, 140, n, step, d.ctypes.data, s.ctypes.data) == _lib.PGX_E_BADARG
        with pytest.raises(pg.ArgumentException):
            pg.pyramid_dims(161, 140, n, step)
    for W, H in [(0, 140), (161, 0), (65536, 140), (161, 65536)]:
        assert L.pgx_pyramid_dims(W, H, 4, 92682, d.ctypes.data, s.ctypes.data) == _lib.PGX_E_BADARG
    assert not d.any() and not s.any()                       # a refused call writes nothing
    assert L.pgx_pyramid_dims(161, 140, 4, 92682, None, None) == _lib.PGX_OK   # either output is optional
    assert L.pgx_pyramid_dims(161, 140, 1, 69632, d.ctypes.data, None) == _lib.PGX_OK and d[0].tolist() == [161, 140]


@pytest.mark.parametrize("step", STEPS)
def test_source_indices_stay_inside(step):
    """q >= 0, x0 <= n_src - 1 (so the clamp of x1 alone keeps both taps inside) and fx in [0, 1), for every source size
    16 ... 300 and the ends of the range of sizes."""
    for n_src in list(range(16, 301)) + [65534, 65535]:
        n_dst = (n_src * 65536) // step
        i0, i1, fr, q = pr.taps(n_dst, n_src, step)
        assert q.min() >= 0 and i0.min() >= 0 and i0.max() <= n_src - 1 and i1.max() <= n_src - 1
        assert (i1 >= i0).all() and fr.dtype == np.float32 and fr.min() >= 0 and fr.max() < 1
        assert (fr.astype(np.float64) * 65536 == (q & 65535)).all()          # the fraction is exact in float32


def test_step_two_is_the_box_mean():
    i0, i1, fr, _ = pr.taps(80, 161, 131072)
    assert i0.tolist() == list(range(0, 160, 2)) and i1.tolist() == list(range(1, 161, 2)) and (fr == 0.5).all()
    g = (np.random.default_rng(0).integers(0, 65536, (48, 64)) / 65535).astype(np.float32)
    box = (g[0::2, 0::2].astype(np.float64) + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2]) / 4
    assert np.abs(pr.down(g, 131072) - box).max() <= 2.0 ** -23              # float32 rounding of three halvings


@pytest.mark.parametrize("step", STEPS)
def test_a_constant_image_stays_bit_identical(step):
    for v in (np.float32(0.37), np.float32(1.0), np.float32(1 / 65535), np.float32(0.0)):
        lv = pr.levels(np.full((140, 161), v, np.float32), 8, step)
        assert sum(l is not None for l in lv) >= 2
        for l in lv:
            assert l is None or (l.view(np.uint32) == np.float32(v).view(np.uint32)).all()


def test_to_level0_keeps_level_0_and_stays_inside():
    x = np.arange(0, 161)
    assert pr.to_level0(x, 65536, 161).tolist() == x.tolist()
    d, s = pr.dims(161, 140, 8, 78643)
    for l in range(8):
        if d[l, 0]:
            got = pr.to_level0(np.arange(d[l, 0]), s[l], 161)
            assert got.min() >= 0 and got.max() <= 160 and (np.diff(got) >= 1).all()      # monotone: no two columns merge


@pytest.fixture(scope="module", params=[5, 6])
def case(request):
    return pr.quality_case(request.param)


def test_the_pyramid_matches_a_half_size_copy_and_one_scale_does_not(case):
    """640 x 480, threshold 0.1, NMS radius 6, gaussian_pairs(0, 8, 256); NN with distance gate 64, ratio 0.8 and cross-check;
    correct = within 2 px of the true position in the half-size image.  Measured: one scale 62 accepted / 0 correct (seed 5)
    and 46 / 1 (seed 6); 4 levels at step 92682: 509 / 455 and 492 / 433.  Both come from the deterministic CPU oracle, so the
    margins only guard against an edit of the test's own inputs."""
    print("single (accepted, correct) =", case["single"], " pyramid =", case["pyramid"])
    assert case["pyramid"][1] >= 300
    assert case["single"][1] <= 10
    st = case["ref_a"]["stats"]
    assert (st[:, 0] > 100).all() and st[:, 0].sum() == case["ref_a"]["count"]           # every level contributes
    lv = case["ref_a"]["origin"][case["sel"][case["sel"][:, 1] >= 0, 0], 0]
    assert np.bincount(lv, minlength=4)[1:].sum() > np.bincount(lv, minlength=4)[0]       # the matches come from the shrunk levels
