"""ec_method_readv_decode and ec_method_writev_rmw on host buffers over the
whole table of tests/_range_sweep.py: every k from 1 to 16 with n = k + 1 and a
wider n up to 31, three masks each, and generated ranges whose clips start and
end inside every row of the stripe.  No GPU is needed: the host variants run on
the calling thread's CPU engine for every gen.

The expected bytes come from the oracle alone, through the case helpers of
_readv_decode_cases.py and _writev_rmw_cases.py.  A read runs with one segment
and cut into three segments of odd lengths with an empty one between them,
each between the 64 guard bytes of tests/test_readv_decode.py; a write runs as
run_case of tests/test_writev_rmw.py does it, in the families "file" and
"arbitrary", with each of the old arrays missing, and in place in the
fragments of the whole file, where every byte outside the window must stay.
"""
import numpy as np
import pytest

import _range_sweep as W
import _writev_rmw_cases as X
import _readv_decode_cases as R
import test_readv_decode as HR
import test_writev_rmw as HW

GENS = HR.GENS


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def test_the_launchers_restated():
    """bucket, waves and the second-trip rows against values worked out by
    hand from ecdk_decode_clip, ecdk_rmw_edge and the row loops."""
    assert [(W.bucket(k), W.waves(k)) for k in (1, 4, 5, 8, 9, 16)] == \
        [(4, 4), (4, 4), (8, 8), (8, 8), (16, 8), (16, 8)]
    assert W.second_trip(4) == [] and W.second_trip(8) == [] and W.second_trip(9) == [8]
    assert W.second_trip(16) == list(range(8, 16))
    assert W.has_encoder(4, 6) and not W.has_encoder(4, 5) and not W.has_encoder(16, 31)
    assert W.clips(2, 1000, 100) == [(1000, 1024), (0, 76)]
    assert W.interior(2, 1000, 100) == (1, 0) and W.interior(2, 1000, 1124)[1] == 1
    assert (W.row_of(511), W.row_of(512)) == (0, 1)
    assert W.inside_row(513) and not W.inside_row(1024)


@pytest.mark.parametrize("seed", [7, 20261021])
def test_other_seeds_keep_the_clauses(seed):
    """table() asserts the geometry clauses and R1...R5 for whatever seed it
    is given."""
    geoms, rs = W.table(seed)
    assert rs != W.RANGES and len(geoms) == len(W.GEOMS)


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", W.GEOMS, ids=W.geom_id)
def test_readv_decode_sweep_host(ec, oracle, geom, gen):
    k, n = geom
    O = W.oracle_for(oracle, k, n)
    before = ec.stats()
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        i = 0
        for mask in W.masks(k, n):
            for head, size in W.RANGES[geom]:
                what = "%d+%d mask %#x range (%d, %d)" % (k, n - k, mask, head, size)
                ins, want = R.case(O, k, n, mask, head, size, W.window(k, head, size, i))
                i += 1
                copies = [f.copy() for f in ins]
                for lengths in ([size], HR.split_lengths(k, head, size)):
                    assert sum(lengths) == size and min(lengths) >= 0
                    bufs, views = HR.segments(lengths)
                    out = views[0] if len(views) == 1 else views
                    assert L.readv_decode(head, mask, ins, out) == 0
                    HR.check_segments(bufs, lengths, want, what)
                for f, c in zip(ins, copies):
                    assert np.array_equal(f, c), what + ": a fragment was written"
    assert ec.stats() == before


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("geom", W.GEOMS, ids=W.geom_id)
def test_writev_rmw_sweep_host(ec, oracle, geom, family, gen):
    k, n = geom
    O = W.oracle_for(oracle, k, n)
    before = ec.stats()
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        i = 0
        for mask in W.masks(k, n):
            for head, size in W.RANGES[geom]:
                what = "%d+%d mask %#x range (%d, %d) %s" % (k, n - k, mask, head, size, family)
                c = X.case(O, k, n, mask, head, size, W.window(k, head, size, i), i, family)
                i += 1
                HW.run_case(L, k, n, head, mask, c, what)
    assert ec.stats() == before


@pytest.mark.parametrize("drop", W.DROPS, ids=lambda d: "no-" + "-".join(d))
@pytest.mark.parametrize("geom", W.GEOMS, ids=W.geom_id)
def test_writev_rmw_sweep_host_missing_old_stripes(ec, oracle, geom, drop):
    k, n = geom
    O = W.oracle_for(oracle, k, n)
    mask = W.masks(k, n)[W.DROPS.index(drop)]
    with ec.ECMatrixList(k, n, gen="none") as L:
        for i, (head, size) in enumerate(W.RANGES[geom]):
            what = "%d+%d mask %#x range (%d, %d) without %s" % (k, n - k, mask, head, size, drop)
            c = X.case(O, k, n, mask, head, size, W.window(k, head, size, i), i, "arbitrary",
                       drop)
            # with both arrays NULL the mask is ignored
            HW.run_case(L, k, n, head, 0 if len(drop) == 2 else mask, c, what)


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", W.GEOMS, ids=W.geom_id)
def test_writev_rmw_sweep_host_in_place(ec, oracle, geom, gen):
    """out[b] points into the fragments of the whole file at chunk `win`, the
    old chunks are the very chunks the call replaces, and every byte outside
    the window stays."""
    k, n = geom
    O = W.oracle_for(oracle, k, n)
    mask = W.masks(k, n)[W.GEOMS.index(geom) % 3]
    bricks = [r - 1 for r in oracle.mask_rows(mask)]
    with ec.ECMatrixList(k, n, gen=gen) as L:
        for i, (head, size) in enumerate(W.RANGES[geom]):
            win = W.window(k, head, size, i)
            last = win + W.stripes(k, head, size) - 1
            user, frags, after = X.in_place(O, k, n, mask, head, size, win, i)
            out = [f[win * W.CHUNK:] for f in frags]
            old_head = [frags[b][win * W.CHUNK:(win + 1) * W.CHUNK] for b in bricks]
            old_tail = [frags[b][last * W.CHUNK:(last + 1) * W.CHUNK] for b in bricks]
            assert old_head[0].ctypes.data == out[bricks[0]].ctypes.data
            assert L.writev_rmw(head, user, mask, old_head, old_tail, out) == 0
            for b, (f, w) in enumerate(zip(frags, after)):
                assert np.array_equal(f, w), \
                    "%d+%d mask %#x range (%d, %d): fragment %d" % (k, n - k, mask, head, size, b)
