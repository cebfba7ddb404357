"""CPU: the caps the certified ID kernel's GPU tests put on its exact-path pixels, proved on the reference
alone. Each capped frame's primary rays (harness.primary_rays, len0 0, the params' max_ray_length) go through the
listed-ray model of the certified walk (cert_rays.model_walks: scripts/certsim.c with the kernel's start checks)
and the oracle's exact march: no certain outcome of the model may differ from the exact walk's, and the pixels the
model leaves to the exact path stay within the frame's cap.

The model's counts of 5184 pixels, each with 0 unsound: terrain 16^3 at ray_noise 0 / 0.05: 3 / 2; glass_cube
16^3: 1 / 3; refraction 16^3: 1 / 1; refraction 64^3 at the lattice camera (0, 10, -8.5) / (-90, 225, 0): 72;
glass_cube 64^3 at (1, 2, -3) / (0, 0, 0): 298. (The whole-frame model, cs_run, has no start checks and reports 2
mismatching primaries at that lattice camera; with the start checks there is none.)"""
import pytest

from ids_cert_model import CAP_DEFAULT, CAP_HARD, H, SCENES, W, model_frame

DEFAULT_FRAMES = [(s, 16, noise, None, None, CAP_DEFAULT) for s in SCENES for noise in (0.0, 0.05)]
HARD_FRAMES = [("refraction", 64, 0.0, (0.0, 10.0, -8.5), (-90.0, 225.0, 0.0), CAP_HARD),
               ("glass_cube", 64, 0.0, (1.0, 2.0, -3.0), (0.0, 0.0, 0.0), CAP_HARD)]


def test_caps_are_shares_of_the_frame():
    assert (CAP_DEFAULT, CAP_HARD) == (51, 518) and W * H == 5184


@pytest.mark.parametrize("name,n,ray_noise,pos,rot,cap", DEFAULT_FRAMES + HARD_FRAMES)
def test_model_is_sound_and_within_the_cap(built, name, n, ray_noise, pos, rot, cap):
    fallback, unsound = model_frame(name, n, ray_noise, pos, rot)
    print(f"{name} {n}^3 noise {ray_noise} camera {pos} {rot}: {fallback} of {W * H} pixels on the exact path "
          f"(cap {cap}), {unsound} unsound")
    assert unsound == 0
    assert 0 <= fallback <= cap
    assert fallback < W * H   # the certified walk settles pixels at all
