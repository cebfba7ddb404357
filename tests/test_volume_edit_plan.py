"""vrt_volume_edit_plan (CPU, host arithmetic): the packed texels an in-place edit
(vrt_update_volume_region) may change. The plan equals its defining formulas, and on small volumes a
brute-force NumPy G / D of the volume before and after seeded edits changes no texel outside it.

Per axis, edit cells [lo, hi), octant step s, FC = kFwdCap, DC = kDistCap: the anchors whose forward
distance F can change are [lo - (FC-1), hi - 1] (s = +1) or [lo, hi - 1 + (FC-1)] (s = -1); the
texel G(w) = F(w - s) - 1 shifts that range by s; united with [lo, hi) for the voxel bytes and
clipped to [0, N). Single layout: [lo - (DC-1), hi - 1 + (DC-1)], clipped.

At N = 16 and 32 the caps' reach exceeds the volume, so every span runs to the volume's face and the
brute-force cases never try the plan's width; the cases that carry the weight are the N = 256 ones on
void256, against the fast reference (tests/skipfield_fast.c), where the plans are strict sub-boxes."""
import numpy as np
import pytest

import voxelraytracer_amd as vrt
from skipfield_reference import (CAP, FWD_CAP, apply_edit, chebyshev_fast, forward_fast, packed_fast,
                                 packed_texels, random_edit, void256)


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
    """At these sizes the caps' reach (127 and 63 cells) exceeds the volume, so no span of the plan is cut by
    a cap (asserted below): the plan is the whole volume in the single layout, and in the octant layout it
    runs from the edit to the faces behind it, leaving out only texels ahead of the edit. The width of the
    plan is never tried here; test_changed_texels_at_256 is the case where it is."""
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
        for o, row in enumerate(plan):   # no span is cut by a cap, every one runs to the volume's face
            for a in range(3):
                if octants == 1 or not o >> a & 1:
                    assert row[a] == 0, (o, a, row)
                if octants == 1 or o >> a & 1:
                    assert row[3 + a] == n, (o, a, row)
        for o, (x0, y0, z0, x1, y1, z1) in enumerate(plan):
            diff = before[o] != after[o]
            assert diff.any(), "an edit that changes emptiness changes texels"
            inside = np.zeros_like(diff)
            inside[z0:z1, y0:y1, x0:x1] = True
            assert not np.any(diff & ~inside), (origin, ext, o, np.argwhere(diff & ~inside)[:4])
        vox, before = new, after


N256 = 256
CENTRE = (128, 128, 128)
EDITS_256 = {   # name: (origin (x, y, z), block [z][y][x]) on void256
    "set_centre": (CENTRE, np.full((1, 1, 1), 1, np.uint8)),
    "set_off_centre": ((200, 150, 90), np.full((1, 1, 1), 1, np.uint8)),
    "carve_floor": ((100, 20, 100), np.zeros((4, 2, 3), np.uint8)),   # 3 x 2 x 4 cells, y = 20 and 21
    "clear_lone": ((10, 10, 10), np.zeros((1, 1, 1), np.uint8)),
}


@pytest.mark.parametrize("octants", [8, 1])
@pytest.mark.parametrize("name", list(EDITS_256))
def test_changed_texels_at_256(built, name, octants):
    """void256 against the fast reference: (a) some octant's plan is a strict sub-range of every axis, so
    the case can fail; (b) no changed texel lies outside the plan; (c) for the voxel set at the centre the
    changed texels touch all six faces of the plan in every octant whose far anchor (127 cells behind the
    edit on every axis) had F = 128 before, which then holds 127; in the single layout, where the cells 63
    away go from D = 64 to 63, five faces (the floor slab keeps D low towards the sixth). The plan is tight:
    it is not an over-wide box hiding an under-wide one."""
    n = N256
    origin, block = EDITS_256[name]
    vox = void256()
    new = apply_edit(vox, n, origin, block)
    assert np.any((new != 0) != (vox != 0))
    before, after = packed_fast(vox, n, octants), packed_fast(new, n, octants)
    ext = block.shape[::-1]
    plan = vrt.volume_edit_plan(n, octants, origin, ext)
    assert len(plan) == octants
    assert any(all(row[a] > 0 or row[3 + a] < n for a in range(3)) for row in plan), plan   # (a)
    boxes = []
    for o, (x0, y0, z0, x1, y1, z1) in enumerate(plan):
        diff = before[o, :n, :n, :n] != after[o, :n, :n, :n]
        assert diff.any(), "an edit that changes emptiness changes texels"
        zz, yy, xx = np.nonzero(diff)
        box = (int(xx.min()), int(yy.min()), int(zz.min()), int(xx.max()) + 1, int(yy.max()) + 1, int(zz.max()) + 1)
        assert all(box[a] >= plan[o][a] and box[3 + a] <= plan[o][3 + a] for a in range(3)), (o, box, plan[o])   # (b)
        inside = np.zeros_like(diff)
        inside[z0:z1, y0:y1, x0:x1] = True
        assert not np.any(diff & ~inside), (origin, ext, o, np.argwhere(diff & ~inside)[:4])
        boxes.append(box)
    if name != "set_centre":
        return
    if octants == 1:   # (c)
        far = CENTRE[0] + (CAP - 1)
        assert chebyshev_fast(vox, n)[far, far, far] == CAP and chebyshev_fast(new, n)[far, far, far] == CAP - 1
        # five faces of the plan are touched; towards the floor slab (y = 20) D(v) <= y - 20 already, and the
        # new voxel is nearer than that only where 128 - y < y - 20, from y = 75 on
        lo, hi = CENTRE[0] - (CAP - 1), CENTRE[0] + CAP
        assert plan == [(lo, lo, lo, hi, hi, hi)] and boxes == [(lo, 75, lo, hi, hi, hi)], (boxes, plan)
        return
    want = []
    for o in range(8):
        ax, ay, az = (CENTRE[a] - (FWD_CAP - 1) * (-1 if o >> a & 1 else 1) for a in range(3))
        f0, f1 = int(forward_fast(vox, n, o)[az, ay, ax]), int(forward_fast(new, n, o)[az, ay, ax])
        if f0 == FWD_CAP:
            assert f1 == FWD_CAP - 1, (o, f0, f1)
            want.append(o)
        else:
            assert f1 == f0, (o, f0, f1)
    # the far anchor's cube holds the floor slab where the y step is +1 (y in [1, 128]), the cluster or the
    # voxel at (10, 10, 10) in octants 0 and 4, and the byte 200 at (245, 200, 30) in octant 3
    assert want == [2, 6, 7], want
    tight = [o for o in range(8) if boxes[o] == tuple(plan[o])]
    assert set(want) <= set(tight), (want, tight, boxes, plan)
