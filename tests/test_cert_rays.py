"""CPU: the certified walk's model (scripts/certsim.c) against the oracle's exact walks, ray by ray, on the
directed ray lists of tests/cert_rays.py: rays through lattice edges and corners, along and out of the volume's
faces, from origins on lattice planes, with length limits that end at the crossing aimed at. A certified walk
returns the exact walk's outcome or says "unsure"; every certain outcome of the model must be the exact walk's,
for the air walk (found, byte, face axis; the hit parameter within the walk's own bound) and the shadow walk
(blocked). The conditions at the end keep the lists from passing empty: they are asserted on the reference side
alone. tests/test_gpu_cert_rays.py holds the kernel to the same oracle on the same rays.

The batched oracle export the lists are marched with (oracle.march_rays) is held to the NumPy oracle first."""
import numpy as np
import pytest

import cert_rays
import oracle
from cert_rays import EXITS, HIT, NOT_STARTED, describe, model_walks, parameter_error, unsound
from harness import float_bits
from oracle import numpy_oracle

REQUIRED_EXITS = ("HIT", "HIT_ONE_FLAG", "EVENT_FLAGS", "EVENT_LEN", "CORNER", "AHEAD", "LEN_MISS", "LEN_TIE",
                  "OUTSIDE")


def numpy_tracer(vox, n, max_len):
    return numpy_oracle.Tracer(vox, n, dict(sun_dir=[0.0, 1.0, 0.0], time=0.0, ray_noise=0.0, reflection_noise=0.0,
                                            refraction_noise=0.0, max_ray_length=max_len, max_reflections=1,
                                            max_transparencies=2, color_only=1))


def test_batched_oracle_matches_numpy_oracle(built):
    """oracle.march_rays against numpy_oracle.Tracer.march / march_shadow (ray dict len = len0) on 300 rays of
    the generator, bit for bit on every field."""
    f = np.float32
    vname, n, dens = "random", 16, 0.12
    vox = cert_rays.volume(vname, n, dens)
    rays = np.concatenate([cert_rays.rays(vname, n, dens, cls)[:50] for cls in cert_rays.CLASSES])
    assert len(rays) == 300
    got = [oracle.march_rays(vox, n, rays, shadow=s) for s in (False, True)]
    nfound = nblocked = 0
    for i, r in enumerate(rays):
        tr = numpy_tracer(vox, n, f(r["max_length"]))
        ray = dict(pos=tuple(f(x) for x in r["origin"]), dir=tuple(f(x) for x in r["dir"]), len=f(r["len0"]),
                   energy=f(1.0), voxel=0, r=0, t=0)
        st = dict(steps=0, flags=0)
        hit = tr.march(dict(ray), st)
        g = got[0][i]
        assert bool(g["found"]) == hit["found"] and g["steps"] == st["steps"] and g["flags"] == st["flags"], (i, g, hit, st)
        if hit["found"]:
            nfound += 1
            assert (g["voxel"], g["index"], g["vidx"]) == (hit["voxel"], hit["index"], hit["vidx"]), (i, g, hit)
            assert float_bits(g["len"])[0] == float_bits(hit["len"])[0], (i, g, hit)
            assert np.array_equal(float_bits(g["point"]), float_bits(np.array(hit["point"], f))), (i, g, hit)
            assert np.array_equal(float_bits(g["normal"]), float_bits(np.array(hit["normal"], f))), (i, g, hit)
        else:
            assert g["vidx"] == -1 and not float_bits(g["len"]).any() and not float_bits(g["point"]).any(), (i, g)
        st = dict(steps=0, flags=0)
        blocked = tr.march_shadow(dict(ray), st)
        s = got[1][i]
        nblocked += bool(blocked)
        assert bool(s["found"]) == bool(blocked) and s["steps"] == st["steps"] and s["flags"] == st["flags"], (i, s, blocked, st)
    assert nfound >= 30 and nblocked >= 30 and nfound <= 270, (nfound, nblocked)


def soundness(rays, exact, got, kind):
    """-> (bool [m]: rays whose certain outcome is not the exact walk's, bool [m]: plain hits whose parameter
    misses the exact length by more than the walk's bound)."""
    off = np.zeros(len(rays), bool)
    if kind == 0:
        plain = (got["res"] == HIT) & (exact["found"] != 0) & (got["exitc"] == EXITS.index("HIT"))
        off = plain & ~(parameter_error(rays, exact, got) <= got["eu"].astype(np.float64))
    return unsound(exact, got, kind), off


TALLY = {}   # (volume id, class, kind) -> the model's exit tallies, filled by the test below


@pytest.mark.parametrize("vol", cert_rays.VOLUMES, ids=cert_rays.volume_id)
def test_model_is_sound_on_directed_rays(built, vol):
    """Every (class, kind) of one volume: zero disagreements between the model's certain outcomes and the exact
    walk's, the plain hits' parameter within eu of the exact length; per volume and kind, found (blocked) and
    missed (lit) rays are each at least 5 % of the list."""
    vname, n, dens = vol
    vox = cert_rays.volume(vname, n, dens)
    shares = {0: [0, 0], 1: [0, 0]}
    failures = []
    for cls in cert_rays.CLASSES:
        rays = cert_rays.rays(vname, n, dens, cls)
        for kind in (0, 1):
            exact = cert_rays.exact_walks(vox, n, rays, kind)
            got = model_walks(vox, n, rays, kind)
            refused = cert_rays.not_started(vox, n, rays, kind)
            assert np.array_equal(got["res"] == NOT_STARTED, refused), (
                cls, kind, "the model's start checks differ from their NumPy restatement",
                np.flatnonzero((got["res"] == NOT_STARTED) != refused)[:5].tolist())
            wrong, off = soundness(rays, exact, got, kind)
            TALLY[(cert_rays.volume_id(vol), cls, kind)] = np.bincount(got["exitc"][got["res"] != NOT_STARTED],
                                                                      minlength=len(EXITS))
            certain = np.count_nonzero(got["res"] <= HIT)
            print(f"{cert_rays.volume_id(vol)} {cls} kind {kind}: certain {certain / len(rays):.3f}, not started "
                  f"{np.count_nonzero(refused)}, disagree {np.count_nonzero(wrong)}, parameter off {np.count_nonzero(off)}")
            if wrong.any():
                failures.append((cls, kind, "certain outcomes that are not the exact walk's", int(wrong.sum()),
                                 describe(rays, exact, got, wrong)))
            if off.any():
                failures.append((cls, kind, "|(len - len0) - u| > eu", int(off.sum()), describe(rays, exact, got, off)))
            shares[kind][0] += int(np.count_nonzero(exact["found"]))
            shares[kind][1] += len(rays)
    assert not failures, failures
    for kind, (nf, total) in shares.items():
        assert 0.05 * total <= nf <= 0.95 * total, (kind, "found / blocked share of the exact walks", nf, total)


def test_directed_rays_reach_the_rare_blocks(built):
    """Over all cases the shadow walk's exits reach each of the walk's blocks at least 50 times (BEHIND is rare by
    construction and is not required)."""
    if len(TALLY) < 2 * len(cert_rays.VOLUMES) * len(cert_rays.CLASSES):   # run alone: fill the tallies
        for vname, n, dens in cert_rays.VOLUMES:
            vox = cert_rays.volume(vname, n, dens)
            for cls in cert_rays.CLASSES:
                got = model_walks(vox, n, cert_rays.rays(vname, n, dens, cls), 1)
                TALLY[(cert_rays.volume_id((vname, n, dens)), cls, 1)] = np.bincount(
                    got["exitc"][got["res"] != NOT_STARTED], minlength=len(EXITS))
    total = sum(t for (_, _, kind), t in TALLY.items() if kind == 1)
    print({name: int(total[i]) for i, name in enumerate(EXITS)})
    for name in REQUIRED_EXITS:
        assert total[EXITS.index(name)] >= 50, (name, int(total[EXITS.index(name)]))
