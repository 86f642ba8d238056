"""ec_method_heal_mixed on host buffers over the whole table of
tests/_heal_mixed_sweep.py: every k from 1 to 16, n up to 31, up to 15 targets
in one to four target words, sources and targets up to brick 30, and the
pattern lists that cross the device kernel's argument space.  No GPU is needed:
the host variant runs on the calling thread's CPU engine for every gen.

The expected fragments come from the oracle alone, through
_heal_mixed_cases.case.  Every fragment lies between the 64 guard bytes of
tests/test_heal_mixed.py, and every byte that is no target chunk of its group
must stay as it was.
"""
import numpy as np
import pytest

import _heal_mixed_cases as C
import _heal_mixed_sweep as W
import test_heal_mixed as H

GENS = H.GENS


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def test_the_launcher_restated():
    """bucket, waves, kw, dw and the pattern words against values worked out
    by hand from ecdk_heal_mixed and HealMixedArgs."""
    assert [(W.bucket(k), W.waves(k)) for k in (1, 4, 5, 8, 9, 16)] == \
        [(4, 4), (4, 4), (8, 8), (8, 8), (16, 8), (16, 8)]
    assert [W.kw(k) for k in (1, 4, 5, 8, 9, 12, 13, 16)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [W.dw(m) for m in (1, 4, 5, 8, 9, 12, 13, 15)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert (C.ARG_HEADER, C.ARG_WORDS) == (304, 436)
    assert [W.pwords(k, 15) for k in (3, 7, 11, 16)] == [21, 37, 53, 69]
    assert [C.ARG_WORDS // w for w in (21, 37, 53, 69)] == [20, 11, 8, 6]
    p = (0b0111, 0b1000)
    c = W.Call(3, 5, [p] * 4, [0] * 3, 9, 4, "x")
    assert W.ngroups(c) == 3 and not W.in_table(c) and W.pwords(3, 1) == 4
    assert W.arg_fit(3, [p] * 200) == 109 and W.in_table(c._replace(pairs=[p] * 110))
    assert W.positions((0b0110100, 0b1001010)) == {"below", "between", "above"}


@pytest.mark.parametrize("seed", [7, 20261021])
def test_other_seeds_keep_the_clauses(seed):
    """table() asserts M1...M7 for whatever seed it is given."""
    other = W.table(seed)
    assert other != W.SWEEP and len(other) == len(W.SWEEP)


def test_k1_decodes_to_its_fragment(oracle):
    """The two facts that stand in for the oracle's decode at k = 1, and that
    nothing else gets the stand-in."""
    for n in (2, 5, 31):
        o = W.oracle_for(oracle, 1, n)
        assert o is not oracle
        f = oracle.fill_xorshift(W.CHUNK, seed=n)
        assert np.array_equal(o.decode(1, [n], [f]), f)
    assert W.oracle_for(oracle, 2, 3) is oracle
    assert {c.k for c in W.SWEEP if c.k == 1} == {1}


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("call", W.SWEEP, ids=W.call_id)
def test_heal_mixed_sweep_host(ec, oracle, call, family, gen):
    c = call
    cs = W.case(oracle, c, family)
    W.check_case(c, cs, family)
    bufs, views = H.guarded(cs.frags)
    before = ec.stats()
    with ec.ECMatrixList(c.k, c.n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        assert L.heal_mixed(c.ns, c.gs, [c.pairs[u][0] for u in c.ids],
                            [c.pairs[u][1] for u in c.ids], views) == 0
    H.check(bufs, cs.want, "%s %s %s" % (W.call_id(c), family, gen))
    assert ec.stats() == before
