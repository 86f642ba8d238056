"""ec_method_heal_checked2 on host buffers over every brick, every pair of
bricks and every k from 2 to 16, with the case builder of tests/
_scrub_sweep.py: per k the lowest k + 4 bricks of a k+5 volume with the last
brick healed, and one drawn mask of k + 6 bricks of a 31-brick volume with two
bricks healed; one call each of 1 + a + C(a, 2) stripes -- clean, every brick,
every pair.

Nothing expected comes from the library: with a - k >= 4 the rule of include/
ec_method.h names every damaged brick and pair (the builder's loc2) and every
target chunk is the chunk the data encodes to.
"""
import numpy as np
import pytest

import _scrub_sweep as W

GENS = ["none", "avx"]


def sweep_geoms():
    """(k, n, avail_mask) per k: k + 4 of k + 5, and k + 6 drawn of 31."""
    out = []
    for k in range(2, 17):
        out.append((k, k + 5, (1 << (k + 4)) - 1))
        out.append((k, 31, W._drawn(k, k + 6, 0, 2)))
    return out


def targets_of(g):
    """The last brick of k + 5; the lowest and the highest brick outside the
    drawn mask."""
    k, n, avail_mask = g
    outside = [b for b in range(n) if not (avail_mask >> b) & 1]
    return [outside[0]] if n == k + 5 else [outside[0], outside[-1]]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", sweep_geoms(), ids=W.geom_id)
def test_heal_checked2_sweep_host(ec, oracle, geom, gen):
    S = W.built(geom)
    assert S.two
    k, n, nst = S.k, S.n, S.nst
    targets = targets_of(geom)
    given = [np.full(W.CHUNK * nst, 0x3C, np.uint8) if f is None else f.copy() for f in S.frags]
    copies = [f.copy() for f in given]
    out = [np.full(W.CHUNK * (nst + 1), W.FILL, np.uint8) for _ in targets]
    loc = np.full(nst + W.GUARD, W.SENTINEL, np.uint32)
    with ec.ECMatrixList(k, n, gen=gen) as L:
        nbad, nmany = L.heal_checked2(nst, S.avail_mask, given, W.mask_of(targets), out, loc)
    assert (nbad, nmany) == (S.ndirty, 0)
    assert (loc[nst:] == W.SENTINEL).all(), "guard words written"
    d = np.flatnonzero(loc[:nst] != S.loc2)
    assert d.size == 0, [(t, S.cases[t], hex(loc[t])) for t in d[:8]]
    for j, o in zip(targets, out):
        assert (o[W.CHUNK * nst:] == W.FILL).all(), "guard chunk written"
        d = np.flatnonzero((o[:W.CHUNK * nst].reshape(nst, W.CHUNK) !=
                            S.clean[j].reshape(nst, W.CHUNK)).any(axis=1))
        assert d.size == 0, (j, [(t, S.cases[t]) for t in d[:8]])
    for b, (f, c) in enumerate(zip(given, copies)):
        assert np.array_equal(f, c), "the buffer of brick %d was written" % b
