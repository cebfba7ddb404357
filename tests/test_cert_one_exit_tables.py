"""CPU: the one-exit form of cert_walk's crossing (csrc/vrt_cert.h) against the form with a return at
every outcome, restated in NumPy / plain Python over exhaustive inputs. The crossing's outcome was a
cascade of tests, each leaving the loop on its own (length test, event, flags at an event, the
shadow walk's one-flag hit, alternatives, outside); it is now decided without a branch for the
plain cases (no length stop, no near-edge flag) and overridden by one rare block, and the loop has
one exit. The result's fields (axis, parameter, bound) are no longer carried through the loop but
recomputed after it from the planes the last crossing did not advance. Each pair of forms below
must agree on every input."""
import itertools

import numpy as np

MISS, HIT, UNSURE, RUN = 0, 1, 2, 3


def old_outcome(shadow, lenstop, tie, ev, lenok, nf, alt_ok, alt_bad, outside):
    """The crossing of the form with ten returns: the first test that fires decides."""
    if lenstop:
        return UNSURE if tie else MISS
    pop = bin(nf).count("1")
    if ev:
        if not lenok:
            return UNSURE
        if nf == 0:
            return HIT
        if shadow and pop == 1:
            ok = True
            if nf & 7:
                ok = alt_ok
            if ok:
                return HIT
        return UNSURE
    if nf and alt_bad:
        return UNSURE
    if outside:
        return MISS
    return RUN


def new_outcome(shadow, lenstop, tie, ev, lenok, nf, alt_ok, alt_bad, outside):
    """The one-exit form: the plain outcome by selects, then the rare block's overrides."""
    res = (HIT if lenok else UNSURE) if ev else (MISS if outside else UNSURE)
    stop = ev or outside
    near = nf != 0  # (the superset test holds whenever a flag is set)
    if lenstop or near:
        if lenstop:
            stop = True
            res = UNSURE if tie else MISS
        elif nf != 0 and ev:
            res = UNSURE
            if shadow and lenok and bin(nf).count("1") == 1:
                ok = True
                if nf & 7:
                    ok = alt_ok
                if ok:
                    res = HIT
        elif nf != 0:
            if alt_bad:
                stop = True
                res = UNSURE
    return res if stop else RUN


def test_crossing_outcome_forms_agree():
    """Every combination of the predicates a crossing evaluates, for both walk kinds and all 64
    near-edge words (combinations that cannot occur together, such as lenstop with lenok, too)."""
    n = 0
    for shadow, lenstop, tie, ev, lenok, alt_ok, alt_bad, outside in itertools.product((False, True), repeat=8):
        for nf in range(64):
            a = old_outcome(shadow, lenstop, tie, ev, lenok, nf, alt_ok, alt_bad, outside)
            b = new_outcome(shadow, lenstop, tie, ev, lenok, nf, alt_ok, alt_bad, outside)
            assert a == b, (shadow, lenstop, tie, ev, lenok, nf, alt_ok, alt_bad, outside, a, b)
            n += 1
    assert n == 256 * 64


def test_every_outcome_occurs_in_the_table():
    """The table is not vacuous: each result is produced by both walk kinds, and the one-flag hit
    only by the shadow walk."""
    seen = {False: set(), True: set()}
    for shadow, lenstop, tie, ev, lenok, alt_ok, alt_bad, outside in itertools.product((False, True), repeat=8):
        for nf in (0, 1, 8, 3, 9):
            seen[shadow].add(new_outcome(shadow, lenstop, tie, ev, lenok, nf, alt_ok, alt_bad, outside))
    assert seen[False] == seen[True] == {MISS, HIT, UNSURE, RUN}
    assert new_outcome(True, False, False, True, True, 8, False, False, False) == HIT
    assert new_outcome(False, False, False, True, True, 8, False, False, False) == UNSURE


def fma32(a, b, c):
    """fma in float32 through float64: the product of two float32 is exact in float64; the sum
    rounds once to float64 and once to float32, the same way in both forms below."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def test_result_fields_recomputed_after_the_loop():
    """In the loop: the axis from the planes, the bound gam_b for all three axes, then the crossed
    axis' bound selected. After the loop: the crossed axis' |1/d| and ed selected first, one fma. The
    same fma on the same operands, so the same bits; the axis and the parameter are re-read from the
    planes a stopping crossing leaves as they were. Ties between planes included."""
    rng = np.random.default_rng(9)
    m = 200000
    sig = rng.uniform(-0.5, 40.0, (m, 3)).astype(np.float32)
    tie = rng.integers(0, 4, m)
    sig[tie == 1, 1] = sig[tie == 1, 0]
    sig[tie == 2, 2] = sig[tie == 2, 1]
    sig[tie == 3] = sig[tie == 3, :1]
    ar = (1.0 / rng.uniform(1e-3, 1.0, (m, 3))).astype(np.float32)
    ed = rng.uniform(0.0, 1e-3, (m, 3)).astype(np.float32)
    q2, a1, c0, b1, b0 = (np.float32(v) for v in (1.1e-7, 9.3e-7, 4.1e-5, 1.9e-7, 1.3e-5))
    s1 = np.minimum(sig[:, 0], np.minimum(sig[:, 1], sig[:, 2]))
    uu = np.maximum(s1, np.float32(0.0))
    A = fma32(fma32(np.full(m, q2), uu, np.full(m, a1)), uu, np.full(m, c0))
    B = fma32(np.full(m, b1), uu, np.full(m, b0))
    a = np.where(sig[:, 0] == s1, 0, np.where(sig[:, 1] == s1, 1, 2))
    for with_ed in (False, True):
        gam = np.stack([fma32(B, ar[:, b], A) + (ed[:, b] if with_ed else np.float32(0.0)) for b in range(3)], 1)
        in_loop = gam[np.arange(m), a]
        ar_a, ed_a = ar[np.arange(m), a], ed[np.arange(m), a]
        g = fma32(B, ar_a, A)
        after = g + ed_a if with_ed else g
        assert np.array_equal(in_loop.view(np.uint32), after.astype(np.float32).view(np.uint32))
    assert np.array_equal(sig[np.arange(m), a], s1)
