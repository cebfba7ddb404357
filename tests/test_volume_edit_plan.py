"""vrt_volume_edit_plan (CPU, host arithmetic): the packed texels an in-place edit
(vrt_update_volume_region) may change. The plan equals its defining formulas, and on small volumes a
brute-force NumPy G / D of the volume before and after seeded edits changes no texel outside it.

Per axis, edit cells [lo, hi), octant step s, FC = kFwdCap, DC = kDistCap: the anchors whose forward
distance F can change are [lo - (FC-1), hi - 1] (s = +1) or [lo, hi - 1 + (FC-1)] (s = -1); the
texel G(w) = F(w - s) - 1 shifts that range by s; united with [lo, hi) for the voxel bytes and
clipped to [0, N). Single layout: [lo - (DC-1), hi - 1 + (DC-1)], clipped."""
import numpy as np
import pytest

import voxelraytracer_amd as vrt
from skipfield_reference import CAP, FWD_CAP, apply_edit, packed_texels, random_edit


def expected_plan(n, octants, origin, extent):
    rows = []
    for o in range(octants):
        lo3, hi3 = [], []
        for a in range(3):
            lo, hi = origin[a], origin[a] + extent[a]
            if octants == 8:
                s = -1 if o >> a & 1 else 1
                a0, a1 = (lo - (FWD_CAP - 1), hi - 1) if s > 0 else (lo, hi - 1 + (FWD_CAP - 1))
                t0, t1 = min(a0 + s, lo), max(a1 + s, hi - 1)
            else:
                t0, t1 = lo - (CAP - 1), hi - 1 + (CAP - 1)
            lo3.append(max(t0, 0))
            hi3.append(min(t1, n - 1) + 1)
        rows.append(tuple(lo3 + hi3))
    return rows


def boxes(n):
    m = n // 2
    return [
        ((m, m, m), (1, 1, 1)),                      # interior, one voxel
        ((m - 7, m + 3, m - 20), (16, 5, 9)),        # interior box
        ((130, 200, 129), (3, 1, 2)),                # interior; at n = 1024 past the caps from every face
        ((0, 0, 0), (1, 1, 1)),                      # corner
        ((0, m, 5), (4, 4, 4)),                      # low x face
        ((n - 3, m, m), (3, 2, 1)),                  # high x face
        ((m, 0, n - 1), (2, 6, 1)),                  # low y, high z faces
        ((10, n - 8, 0), (100, 8, 128)),             # wide box on two faces
        ((0, 0, 0), (n, n, n)),                      # the whole volume
        ((0, 0, 0), (n, 1, n)),                      # a whole slab
    ]


@pytest.mark.parametrize("octants", [8, 1])
@pytest.mark.parametrize("n", [256, 1024])
def test_plan_equals_the_formulas(built, n, octants):
    for origin, extent in boxes(n):
        plan = vrt.volume_edit_plan(n, octants, origin, extent)
        assert len(plan) == octants
        assert plan == expected_plan(n, octants, origin, extent), (origin, extent)
        for row in plan:   # half-open, non-empty, inside [0, n)^3, holds the edit box
            for a in range(3):
                assert 0 <= row[a] <= origin[a] and origin[a] + extent[a] <= row[3 + a] <= n


def test_plan_interior_sizes(built):
    """A one-voxel edit far from every face: 128 texels per axis per octant (the work bound of the
    regional rebuild), 127 per axis in the single layout."""
    for row in vrt.volume_edit_plan(512, 8, (256, 256, 256), (1, 1, 1)):
        assert [row[3 + a] - row[a] for a in range(3)] == [FWD_CAP] * 3
    (row,) = vrt.volume_edit_plan(512, 1, (256, 256, 256), (1, 1, 1))
    assert [row[3 + a] - row[a] for a in range(3)] == [2 * CAP - 1] * 3


@pytest.mark.parametrize("args", [(256, 8, (0, 0, 0), (0, 1, 1)), (256, 8, (0, 0, 0), (1, -1, 1)),
                                  (256, 8, (255, 0, 0), (2, 1, 1)), (256, 8, (-1, 0, 0), (1, 1, 1)),
                                  (256, 8, (0, 256, 0), (1, 1, 1)), (256, 4, (0, 0, 0), (1, 1, 1)),
                                  (100, 8, (0, 0, 0), (1, 1, 1)), (2048, 1, (0, 0, 0), (1, 1, 1))])
def test_plan_rejects_bad_arguments(built, args):
    with pytest.raises(vrt.VrtError) as e:
        vrt.volume_edit_plan(*args)
    assert e.value.code == vrt.abi.VRT_ERR_INVALID


@pytest.mark.parametrize("octants", [8, 1])
@pytest.mark.parametrize("scene,n,seed", [("terrain", 16, 3), ("refraction", 16, 2), ("glass_cube", 16, 7),
                                          ("terrain", 32, 10), ("refraction", 32, 11)])
def test_every_changed_texel_lies_inside_the_plan(built, scene, n, seed, octants):
    rng = np.random.default_rng(seed)
    vox = vrt.build_scene(scene, n)
    before = packed_texels(vox, n, octants)
    for _ in range(4):   # cumulative edits
        origin, block = random_edit(rng, n)
        new = apply_edit(vox, n, origin, block)
        # an edit that changes no cell's emptiness shows nothing: the seeds are chosen so that none does
        assert np.any((new != 0) != (vox != 0)), "seed draws an edit that changes no emptiness"
        after = packed_texels(new, n, octants)
        ext = block.shape[::-1]
        plan = vrt.volume_edit_plan(n, octants, origin, ext)
        assert len(plan) == octants
        for o, (x0, y0, z0, x1, y1, z1) in enumerate(plan):
            diff = before[o] != after[o]
            assert diff.any(), "an edit that changes emptiness changes texels"
            inside = np.zeros_like(diff)
            inside[z0:z1, y0:y1, x0:x1] = True
            assert not np.any(diff & ~inside), (origin, ext, o, np.argwhere(diff & ~inside)[:4])
        vox, before = new, after
