"""ec_method_decode_verified and ec_method_heal_verified on host buffers over
the whole table of tests/_verified_sweep.py: every k from 1 to 16, check-row
counts 1 to 15 and 18, drawn avail_masks, targets below, between and above the
basis bricks.  No GPU is needed: the host entry points run on the calling
thread's CPU engine for every gen.

The expected values come from the oracle and the rule in include/ec_method.h,
never from the library.  Every output is pre-filled with 0xA5 and followed by
a guard chunk, bad[] with 0xFFFFFFFF and guard words; no fragment may change,
nor the buffer of any brick outside avail_mask.
"""
import numpy as np
import pytest

import _verified_sweep as W

GENS = ["none", "avx"]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def test_the_launcher_restated():
    """bucket, waves and items against values worked out by hand from
    launch_scrub_tile and scrub_verified."""
    assert [(W.bucket(k), W.waves(k)) for k in (4, 5, 8, 9)] == [(4, 4), (8, 8), (8, 8), (16, 8)]
    assert W.waves(6, (1 << 17) + 5) == 4 and W.waves(6, 1 << 17) == 8
    assert W.waves(3, 1 << 20) == 4 and W.waves(12, 1 << 20) == 8
    assert [W.kw(k) for k in (1, 4, 5, 8, 9, 12, 13, 16)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert W.items((2, 3, 0x7, ())) == 3                            # 1 check row + 2
    g = (4, 6, 0x1F, ((5,),))
    assert (W.nrows(g), W.items(g), W.items(g, (5,))) == (1, 5, 2)
    g = (16, 31, W.ALL31, ())
    assert (W.nrows(g), W.items(g), W.table_words(g)) == (15, 31, 124)
    g = (13, 31, 0x3FFF, (tuple(range(14, 31)),))
    assert (W.items(g, g[3][0]), W.table_words(g, g[3][0])) == (18, 72)
    g = (4, 6, 0x3D, ((1,),))
    assert W.split(g) == ([0, 2, 3, 4], [5]) and W.position(g, 1) == "between"


@pytest.mark.parametrize("seed", [7, 20261021])
def test_other_seeds_keep_the_clauses(seed):
    """table() asserts V1...V7 for whatever seed it is given."""
    other = W.table(seed)
    assert other != W.SWEEP and len(other) == len(W.SWEEP)


@pytest.mark.parametrize("k", [3, 7, 11])
def test_expectation_obeys_the_mds_rules(oracle, k):
    """One geometry per K bucket: the expectation against the rule, restated
    from the list of cases alone (build() derives it from the bytes)."""
    g = [x for x in W.offset_geoms() if x[0] == k][0]
    S = W.built(g)
    r = len(S.checks)
    assert S.nst == 1 + (k + r) + r * (r - 1) // 2 + r + 1
    kc = k * W.CHUNK
    for t, case in enumerate(S.cases):
        hit = any(b in S.basis for b in case)
        assert S.bad[t] == (S.cmask if hit else W.mask_of(case)), (t, case)
        same = np.array_equal(S.out[t * kc:(t + 1) * kc], S.data[t * kc:(t + 1) * kc])
        assert same == (not hit), (t, case)
        for j in g[3][2]:
            assert np.array_equal(W.chunk(S.enc[j], t), W.chunk(S.clean[j], t)) == (not hit)
    assert S.nbad == S.nst - 1 and {len(c) for c in S.cases} == {0, 1, 2}


def run_host(L, S, targets):
    """One host call of a geometry: (bad, outputs, nbad), guards checked."""
    nst, k = S.nst, S.k
    per = W.CHUNK * (k if targets is None else 1)
    # bricks outside avail_mask, the targets among them, get a buffer of their
    # own in frags[]: nothing may read or write it
    given = [np.full(W.CHUNK * nst, 0x3C, np.uint8) if f is None else f for f in S.frags]
    copies = [f.copy() for f in given]
    out = [np.full(per * nst + W.CHUNK, W.FILL, np.uint8) for _ in (targets or (0,))]
    bad = np.full(nst + W.GUARD, W.SENTINEL, np.uint32)
    if targets is None:
        nbad = L.decode_verified(nst, S.avail_mask, given, out[0], bad)
    else:
        nbad = L.heal_verified(nst, S.avail_mask, given, W.mask_of(targets), out, bad)
    assert (bad[nst:] == W.SENTINEL).all(), "guard words written"
    for o in out:
        assert (o[per * nst:] == W.FILL).all(), "guard chunk written"
    for b, (f, c) in enumerate(zip(given, copies)):
        assert np.array_equal(f, c), "the buffer of brick %d was written" % b
    return bad[:nst], [o[:per * nst] for o in out], nbad


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", W.SWEEP, ids=W.geom_id)
def test_verified_sweep_host(ec, oracle, geom, gen):
    S = W.built(geom)
    with ec.ECMatrixList(S.k, S.n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        for targets in (None,) + S.heals:
            bad, outs, nbad = run_host(L, S, targets)
            W.compare(S, targets, bad, outs, nbad, (W.geom_id(geom), gen, targets))
