"""The fast reference of the skip field (tests/skipfield_fast.c through tests/skipfield_reference.py, CPU):
equal to the brute-force NumPy reference in every texel of both layouts at N <= 32, equal to closed forms
at N = 256, where the brute force cannot reach and the caps clamp, and in step with the caps of the
kernels. tests/test_gpu_skipfield_caps.py and tests/test_volume_edit_plan.py hold the kernels and the edit
plan to it at N = 256."""
import os
import re

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from adversarial_volumes import NAMES, volumes
from skipfield_reference import (CAP, FWD_CAP, UNCAPPED, chebyshev_fast, chebyshev_reference, forward_fast,
                                 forward_reference, packed_fast, packed_reference, void256)

CSRC = os.path.join(os.path.dirname(os.path.abspath(vrt.__file__)), "csrc")
DENSITIES = (0.0, 0.002, 0.05, 0.5)
SCENES = ("terrain", "glass_cube", "refraction")


def assert_same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [int(got[tuple(b)]) for b in bad[:4]],
                           [int(want[tuple(b)]) for b in bad[:4]])


def small_volumes(n):
    """(name, n^3 bytes): the built scenes (N >= 8), the adversarial volumes and random volumes."""
    out = [(s, vrt.build_scene(s, n)) for s in SCENES if n >= 8]
    out += [(name, volumes(n)[name]) for name in NAMES]
    rng = np.random.default_rng(1000 + n)
    for dens in DENSITIES:
        v = np.where(rng.random(n ** 3) < dens, rng.integers(1, 256, n ** 3), 0).astype(np.uint8)
        out.append((f"random {dens}", v))
    return out


# ---- fast equals brute force ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 4, 8, 16, 32])
def test_fast_equals_brute_force(built, n):
    """Every texel of the (N+1)^3 volume(s), both layouts; below 32 F and D themselves too."""
    for name, vox in small_volumes(n):
        for octants in (8, 1):
            assert_same(packed_fast(vox, n, octants), packed_reference(vox, n, octants), (name, n, octants))
        if n == 32:   # the brute force is slow there; the packed texels above hold the same values
            continue
        assert_same(chebyshev_fast(vox, n), chebyshev_reference(vox, n), (name, n, "D"))
        for o in range(8):   # G of the brute force from the fast F, shifted here in NumPy
            sl = tuple(slice(None, None, -1) if o >> a & 1 else slice(None) for a in (2, 1, 0))
            f = forward_fast(vox, n, o)[sl].astype(np.int64)
            g = np.zeros((n, n, n), np.int64)
            g[1:, 1:, 1:] = np.maximum(f[:-1, :-1, :-1] - 1, 0)
            assert_same(g[sl], forward_reference(vox, n, o), (name, n, "G", o))


def test_random_volumes_are_what_they_say(built):
    for n in (8, 32):
        filled = [int(np.count_nonzero(v)) for name, v in small_volumes(n) if name.startswith("random")]
        assert filled[0] == 0 and 0 < filled[2] < filled[3] < n ** 3, filled


# ---- closed forms at N = 256 ---------------------------------------------------------------------

N = 256


def face_terms(o):
    """Per axis (z, y, x order of the arrays) the distance to the far face along the octant's step, as
    broadcastable [N] aranges: N - c for step +1, c + 1 for step -1."""
    c = np.arange(N, dtype=np.int16)
    t = [(c + 1) if o >> a & 1 else (N - c) for a in (2, 1, 0)]
    return t[0][:, None, None], t[1][None, :, None], t[2][None, None, :]


@pytest.mark.parametrize("cap", [FWD_CAP, UNCAPPED])
def test_empty_256_forward(built, cap):
    vox = np.zeros(N ** 3, np.uint8)
    for o in range(8):
        tz, ty, tx = face_terms(o)
        want = np.minimum(cap, np.minimum(np.minimum(tz, ty), tx))
        assert_same(forward_fast(vox, N, o, cap), want, ("empty F", o, cap))
    assert int(forward_fast(vox, N, 0, UNCAPPED).max()) == UNCAPPED   # the anchor (0, 0, 0): 256, clamped


@pytest.mark.parametrize("cap", [CAP, UNCAPPED])
def test_empty_256_centred(built, cap):
    c = np.arange(N, dtype=np.int16)
    t = np.minimum(c + 1, N - c)
    want = np.minimum(cap, np.minimum(np.minimum(t[:, None, None], t[None, :, None]), t[None, None, :]))
    got = chebyshev_fast(np.zeros(N ** 3, np.uint8), N, cap)
    assert_same(got, want, ("empty D", cap))
    assert int(got.max()) == min(cap, N // 2)


@pytest.mark.parametrize("u", [(128, 128, 128), (200, 150, 90), (0, 255, 3)])
def test_one_voxel_256(built, u):
    """One occupied voxel u = (x, y, z) in a void: F(v) = min(cap, face term, max_a |u_a - v_a|) where u
    lies in v's forward octant (u_a - v_a has the step's sign or is 0 on every axis), the face term alone
    elsewhere; D(v) = min(cap, face term, max_a |u_a - v_a|) everywhere."""
    vox = np.zeros((N, N, N), np.uint8)
    vox[u[2], u[1], u[0]] = 7
    c = np.arange(N, dtype=np.int16)
    dz, dy, dx = (u[2] - c)[:, None, None], (u[1] - c)[None, :, None], (u[0] - c)[None, None, :]
    cheb = np.maximum(np.maximum(np.abs(dz), np.abs(dy)), np.abs(dx))
    t = np.minimum(c + 1, N - c)
    face = np.minimum(np.minimum(t[:, None, None], t[None, :, None]), t[None, None, :])
    assert_same(chebyshev_fast(vox, N), np.minimum(CAP, np.minimum(face, cheb)), ("one voxel D", u))
    for o in range(8):
        s = [-1 if o >> a & 1 else 1 for a in (2, 1, 0)]   # z, y, x steps
        ahead = (dz * s[0] >= 0) & (dy * s[1] >= 0) & (dx * s[2] >= 0)
        tz, ty, tx = face_terms(o)
        face_o = np.minimum(np.minimum(tz, ty), tx)
        for cap in (FWD_CAP, UNCAPPED):
            want = np.minimum(cap, np.where(ahead, np.minimum(face_o, cheb), face_o))
            assert_same(forward_fast(vox, N, o, cap), want, ("one voxel F", u, o, cap))


def test_packed_256_is_the_shifted_forward_distance(built):
    """sf_packed's own G shift and plane-N rule at N = 256, against sf_forward / sf_chebyshev shifted in
    NumPy, on void256."""
    vox = void256()
    v = vox.reshape(N, N, N)
    wrap = np.arange(N + 1) % N
    for octants in (8, 1):
        got = packed_fast(vox, N, octants)
        assert got.shape == (octants,) + (N + 1,) * 3 and got.dtype == np.uint16
        for o in range(octants):
            want = v[np.ix_(wrap, wrap, wrap)].astype(np.uint16)
            if octants == 8:
                sl = tuple(slice(None, None, -1) if o >> a & 1 else slice(None) for a in (2, 1, 0))
                f = forward_fast(vox, N, o)[sl]
                g = np.zeros((N, N, N), np.uint16)
                g[1:, 1:, 1:] = np.maximum(f[:-1, :-1, :-1].astype(np.int16) - 1, 0)
                skip = g[sl]
            else:
                skip = chebyshev_fast(vox, N).astype(np.uint16)
            want[:N, :N, :N] |= skip << 8
            assert_same(got[o], want, ("packed", octants, o))


def test_void256_makes_the_caps_clamp(built):
    """The floors of tests/test_gpu_skipfield_caps.py, on the reference: uncapped F exceeds 128 and
    uncapped D exceeds 64 in void256, and the capped field holds G = 127 and D = 64."""
    vox = void256()
    for o in range(8):
        f = forward_fast(vox, N, o, UNCAPPED)
        assert int(f.max()) > FWD_CAP and np.count_nonzero(f > FWD_CAP) > 100000, (o, int(f.max()))
        assert_same(forward_fast(vox, N, o), np.minimum(f, FWD_CAP), ("the cap is a clamp", o))
    d = chebyshev_fast(vox, N, UNCAPPED)
    assert int(d.max()) > CAP and np.count_nonzero(d > CAP) > 100000, int(d.max())
    assert_same(chebyshev_fast(vox, N), np.minimum(d, CAP), "the cap is a clamp")
    assert int((packed_fast(vox, N, 8) >> 8).max()) == FWD_CAP - 1
    assert int((packed_fast(vox, N, 1) >> 8).max()) == CAP


# ---- parity with the kernels' constants ----------------------------------------------------------

def test_caps_equal_the_kernels_constants(built):
    """FWD_CAP and CAP are the source's: parsed from csrc/vrt_tuning.h and csrc/vrt_walk.h, and seen through
    the edit plan's interior size, which the library computes from kFwdCap and kDistCap."""
    with open(os.path.join(CSRC, "vrt_tuning.h")) as f:
        tuning = f.read()
    with open(os.path.join(CSRC, "vrt_walk.h")) as f:
        walk = f.read()
    assert re.search(r"constexpr\s+uint32_t\s+kFwdCap\s*=\s*VRT_FWD_CAP\s*;", tuning)
    (fwd,) = re.findall(r"^#define\s+VRT_FWD_CAP\s+(\d+)\s*$", tuning, re.M)
    (dist,) = re.findall(r"constexpr\s+uint32_t\s+kDistCap\s*=\s*(\d+)\s*;", walk)
    assert (int(fwd), int(dist)) == (FWD_CAP, CAP)
    for row in vrt.volume_edit_plan(512, 8, (256, 256, 256), (1, 1, 1)):
        assert [row[3 + a] - row[a] for a in range(3)] == [FWD_CAP] * 3
    (row,) = vrt.volume_edit_plan(512, 1, (256, 256, 256), (1, 1, 1))
    assert [row[3 + a] - row[a] for a in range(3)] == [2 * CAP - 1] * 3
