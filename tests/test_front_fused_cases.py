"""The scenes of tests/front_fused_cases.py are what tests/test_gpu_front_fused.py takes them for (no GPU), asserted on the
oracle alone: every tile of every size has hits in its first and last row and column (so every tile edge and halo column
decides a hit), the maps named for entries outside the image have some and the others none, and every frame that is not flat
leaves enough survivors for the comparison of the lists to mean something.  Every size, map and frame is checked: none is
skipped or sampled."""
import numpy as np
import pytest

import front_fused_cases as ff
import front_limits_cases as fc
from oracle import cref

OUTSIDE = {"none": 0, "identity": 0, "wrap": 0, "flip": 0}    # entries outside the image; shift and halo: see below


def _raw(w, h, kind):
    frames, dmap, _ = ff.scene(w, h, kind)
    return [cref.detect(cref.gray(ff.dewarp(f, dmap)), ff.T) for f in frames]


def test_sizes_and_batches_reach_both_sides_of_the_tile_and_of_the_frame_group():
    assert (ff.TW, ff.TH, ff.HALO) == (64, 32, 3)
    tiles = {(w, h): ((w + 63) // 64, (h + 31) // 32) for w, h in ff.SIZES}
    assert tiles == {(6, 6): (1, 1), (7, 7): (1, 1), (64, 32): (1, 1), (65, 33): (2, 2), (83, 60): (2, 2), (200, 131): (4, 5)}
    assert {1, 3, 5, 9} <= set(ff.BATCHES) and {ff.FG - 1, ff.FG, ff.FG + 1} <= set(ff.BATCHES)
    assert all(w % 64 and h % 32 for w, h in ff.SIZES[-2:])                  # ragged both ways


@pytest.mark.parametrize("kind", ff.MAPS)
@pytest.mark.parametrize("w,h", ff.SIZES)
def test_entries_outside_the_image_where_the_map_is_named_for_them(w, h, kind):
    dmap = ff.make_map(kind, w, h)
    if kind == "none":
        assert dmap is None
        return
    assert dmap.shape == (h, w, 2) and dmap.dtype == np.int32
    bad = ff.outside(dmap)
    if kind == "shift":                                                      # whole border rows and columns
        assert bad[:2].all() and bad[:, w - 5:].all() and bad.sum() == 2 * w + 5 * h - 10
    elif kind == "halo":                                                     # one entry, in the halo of tile (0, 0) where there is one
        hx, hy = ff.halo_pixel(w, h)
        assert bad.sum() == 1 and bad[hy, hx]
        if w > 66 and h > 34:
            assert 64 <= hx < 64 + ff.HALO and 32 <= hy < 32 + ff.HALO
            tile0 = bad[:32 + ff.HALO, :64 + ff.HALO]
            assert tile0.sum() == 1 and not tile0[:32, :64].any()            # tile (0, 0) gathers it, and only for its halo
    else:
        assert bad.sum() == OUTSIDE[kind]
    if bad.any():
        with pytest.raises(cref.OracleError):
            cref.apply_distortion(ff.frames_of(w, h)[0], dmap)
    if kind == "wrap":                                                       # entries below 0 and above 65535, all back inside
        assert (dmap[..., 0] < 0).sum() >= w * h // 4 and (dmap[..., 1] >= 65536).sum() >= w * h // 6
        back = ff.dewarp(ff.frames_of(w, h)[0], dmap)
        assert back.tobytes() == ff.frames_of(w, h)[0][:, ::-1].tobytes()    # the mirrored frame
    if kind == "flip":
        assert ff.dewarp(ff.frames_of(w, h)[1], dmap).tobytes() == ff.frames_of(w, h)[1][::-1, ::-1].tobytes()   # the dense frame
        assert (np.diff(dmap[0, :, 0]) == -1).all() and (np.diff(dmap[:, 0, 1]) == -1).all()   # descending sources


@pytest.mark.parametrize("kind", ff.MAPS)
@pytest.mark.parametrize("w,h", ff.SIZES)
def test_every_tile_has_hits_in_its_first_and_last_row_and_column(w, h, kind):
    raw = _raw(w, h, kind)
    dense = [raw[i] for i in ff.DENSE]
    noise = [raw[i] for i in range(ff.F_MAX) if i not in ff.FLAT + ff.DENSE]
    # the columns and rows FAST can hit at all: 3 .. w - 4 and 3 .. h - 4
    xlo, xhi, ylo, yhi = 3, w - 4, 3, h - 4
    if xlo > xhi or ylo > yhi:
        assert all(len(r) == 0 for r in raw)                                 # 6 x 6: no interior pixel
        return
    if kind == "shift":
        xhi = w - 6                                                          # the last column that is not black
    if (w, h) == (7, 7):                                                     # one candidate, (3, 3)
        assert all(len(r) <= 1 for r in raw)
        if kind != "shift":                                                  # the dense pattern makes it a hit, moved or not
            assert all(len(r) == 1 and (r["x"][0], r["y"][0]) == (3, 3) for r in dense)
        return
    for name, lists in (("dense", dense), ("noise4", noise)):
        xs = np.concatenate([r["x"] for r in lists])
        ys = np.concatenate([r["y"] for r in lists])
        for tx in range((w + 63) // 64):
            for ty in range((h + 31) // 32):
                x0, x1 = max(tx * 64, xlo), min(tx * 64 + 63, xhi)
                y0, y1 = max(ty * 32, ylo), min(ty * 32 + 31, yhi)
                if x0 > x1 or y0 > y1:
                    continue                                                 # a tile of border pixels only
                inside = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
                for edge in ((xs == x0), (xs == x1), (ys == y0), (ys == y1)):
                    assert (inside & edge).any(), (name, tx, ty)
    if kind == "shift" and w > 16 and h > 16:                                # hits whose ring reaches into the zero edge
        for r in dense + noise:
            assert ((r["x"] >= w - 8) | (r["y"] <= 4)).sum() >= 3


@pytest.mark.parametrize("kind", ff.MAPS)
@pytest.mark.parametrize("w,h", ff.SIZES)
def test_survivors(w, h, kind):
    frames, dmap, exp = ff.scene(w, h, kind)
    assert len(exp) == ff.F_MAX == 9
    for i, (kept, desc, n_raw) in enumerate(exp):
        assert len(kept) <= n_raw < ff.RAW and len(kept) < ff.CAP and desc.shape == (len(kept), 8)
        if i in ff.FLAT:                                                     # flat; the halo map's one black pixel is a hit of its own
            hx, hy = ff.halo_pixel(w, h)
            assert n_raw == (kind == "halo" and 3 <= hx <= w - 4 and 3 <= hy <= h - 4)
        elif (w - 6) * (h - 6) >= 100 and i not in ff.FLAT:
            assert len(kept) >= 10, (i, len(kept))
    if (w - 6) * (h - 6) >= 100:
        assert len({e[0].tobytes() for i, e in enumerate(exp) if i not in ff.FLAT}) >= 5   # the frames of a batch differ
    # the 8-bit batch is the same batch
    assert ((frames // 257).astype(np.uint8).astype(np.uint16) * 257 == frames).all()


def test_replacing_the_map_changes_the_lists():
    for w, h in ((83, 60), (65, 33)):
        a, b, c = (ff.scene(w, h, k)[2] for k in ("flip", "shift", "none"))
        for f in (0, 1):
            assert fc.lists_differ(a[f], b[f]) and fc.lists_differ(b[f], c[f]) and fc.lists_differ(a[f], c[f])
