"""The eight scrub entry points on host buffers over every brick, every pair
of bricks and every k from 2 to 16 (tests/_scrub_sweep.py): verify, locate,
locate2, decode_checked, decode_checked2, heal_checked, repair and repair2,
one call each per geometry, on 1 + a + C(a, 2) stripes that damage each brick
and each pair of bricks of avail_mask once.  No GPU is needed: the host entry
points run on the calling thread's CPU engine for every gen.

The expected values come from the oracle and include/ec_method.h, never from
the library.  loc[] / bad[] are pre-filled with 0xFFFFFFFF and followed by
guard words, outputs with 0xA5 and a guard chunk; the fragments, and a buffer
given for every brick outside avail_mask, are compared with their bytes from
before after each call that must not write them; the counters are checked
against counts taken from the expected arrays.
"""
import numpy as np
import pytest

import _scrub_sweep as W

GENS = ["none", "avx"]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def new_loc(nst):
    return np.full(nst + W.GUARD, W.SENTINEL, np.uint32)


def read_loc(loc, nst):
    assert (loc[nst:] == W.SENTINEL).all(), "guard words written"
    return loc[:nst]


def new_out(chunks):
    return np.full(W.CHUNK * (chunks + 1), W.FILL, np.uint8)


def read_out(out, chunks):
    assert (out[W.CHUNK * chunks:] == W.FILL).all(), "guard chunk written"
    return out[:W.CHUNK * chunks]


def same_loc(got, want, S, what):
    d = np.flatnonzero(got != want)
    assert d.size == 0, (what, [(t, S.cases[t], hex(got[t]), hex(want[t])) for t in d[:8]])


def same_stripes(got, want, width, S, what):
    d = np.flatnonzero((got.reshape(S.nst, width) != want.reshape(S.nst, width)).any(axis=1))
    assert d.size == 0, (what, [(t, S.cases[t]) for t in d[:8]])


def given_buffers(S, frags):
    """Writable copies of the fragments; a brick outside avail_mask gets a
    buffer of its own that nothing may read or write."""
    return [np.full(W.CHUNK * S.nst, 0x3C, np.uint8) if f is None else f.copy() for f in frags]


def same_fragments(given, want, S, what):
    for b, (f, w) in enumerate(zip(given, want)):
        if w is None:
            assert (f == 0x3C).all(), (what, "the buffer of brick %d was written" % b)
        else:
            same_stripes(f, w, W.CHUNK, S, (what, "brick %d" % b))


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", W.SWEEP, ids=W.geom_id)
def test_scrub_sweep_host(ec, geom, gen):
    S = W.built(geom)
    k, n, nst, am = S.k, S.n, S.nst, S.avail_mask
    targets = W.targets_of(geom)
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        fr = given_buffers(S, S.frags)

        bad = new_loc(nst)
        nbad = L.verify(nst, W.mask_of(S.basis), [fr[b] for b in S.basis],
                        W.mask_of(S.checks), [fr[b] for b in S.checks], bad)
        same_loc(read_loc(bad, nst), S.bad, S, "verify")
        assert nbad == np.count_nonzero(S.bad)
        same_fragments(fr, S.frags, S, "verify")

        loc = new_loc(nst)
        nbad = L.locate(nst, am, fr, loc)
        same_loc(read_loc(loc, nst), S.loc1, S, "locate")
        assert nbad == S.nbad
        same_fragments(fr, S.frags, S, "locate")

        loc, out = new_loc(nst), new_out(k * nst)
        assert L.decode_checked(nst, am, fr, out, loc) == (S.nbad, S.nmany)
        same_loc(read_loc(loc, nst), S.loc1, S, "decode_checked loc")
        same_stripes(read_out(out, k * nst), S.out1, k * W.CHUNK, S, "decode_checked out")
        same_fragments(fr, S.frags, S, "decode_checked")

        if targets:
            loc, outs = new_loc(nst), [new_out(nst) for _ in targets]
            assert L.heal_checked(nst, am, fr, W.mask_of(targets), outs, loc) == (S.nbad, S.nmany)
            same_loc(read_loc(loc, nst), S.loc1, S, "heal_checked loc")
            for j, o in zip(targets, outs):
                same_stripes(read_out(o, nst), S.heal1[j], W.CHUNK, S, ("heal_checked", j))
            same_fragments(fr, S.frags, S, "heal_checked")

        if S.two:
            loc = new_loc(nst)
            assert L.locate2(nst, am, fr, loc) == S.ndirty
            same_loc(read_loc(loc, nst), S.loc2, S, "locate2")
            same_fragments(fr, S.frags, S, "locate2")

            loc, out = new_loc(nst), new_out(k * nst)
            assert L.decode_checked2(nst, am, fr, out, loc) == (S.ndirty, 0)
            same_loc(read_loc(loc, nst), S.loc2, S, "decode_checked2 loc")
            same_stripes(read_out(out, k * nst), S.data, k * W.CHUNK, S, "decode_checked2 out")
            same_fragments(fr, S.frags, S, "decode_checked2")

        # repair on locate's answer, then a second locate: zero wherever a
        # brick was named, as before elsewhere
        loc1 = S.loc1.copy()
        assert L.repair(nst, am, fr, loc1) == (S.nsingle1, S.nmany)
        assert np.array_equal(loc1, S.loc1), "repair wrote loc"
        same_fragments(fr, S.rep1, S, "repair")
        loc = new_loc(nst)
        L.locate(nst, am, fr, loc)
        same_loc(read_loc(loc, nst), np.where(S.loc1 == W.MANY, S.loc1, 0), S,
                 "locate after repair")

        # repair2 on the bits of the damaged bricks (locate2's answer where
        # it can run): every fragment is the clean one again
        fr = given_buffers(S, S.frags)
        loc2 = S.loc2.copy()
        assert L.repair2(nst, am, fr, loc2) == (S.ndirty, 0)
        assert np.array_equal(loc2, S.loc2), "repair2 wrote loc"
        same_fragments(fr, [S.clean[b] if f is not None else None
                            for b, f in enumerate(S.frags)], S, "repair2")
        if S.two:
            loc = new_loc(nst)
            assert L.locate2(nst, am, fr, loc) == 0
            assert not read_loc(loc, nst).any(), "locate2 after repair2"

            # and with k + 2 of the bricks, on the pairs that lie inside them
            fr = given_buffers(S, S.frags)
            assert L.repair2(nst, S.sub_mask, fr, S.loc_sub.copy()) == \
                (np.count_nonzero(S.loc_sub), 0)
            same_fragments(fr, S.rep_sub, S, "repair2 on k + 2 bricks")
