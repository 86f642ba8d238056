"""ec_method_readv_decode_device and ec_method_writev_rmw_device over the whole
table of tests/_range_sweep.py: ec_decode_clip and ec_rmw_edge with the
run-time k at every value of each K bucket (1...4, 5...8, 9...16), so that the
row loops and the staging are ragged at K = 16 too, n below, at and above the
block's wave count and up to 31 (the encode loop of ec_rmw_edge and, for the
interior, the combine with rows = n), and clips that start and end inside
every row of the stripe, those of a wave's second trip among them.

The expected bytes come from the oracle alone.  The calls of one (geometry,
mask) are queued on one side stream by run_cases of
tests/test_gpu_readv_decode.py and tests/test_gpu_writev_rmw.py: dst and every
out[i] lie between two 2 KiB guards of 0xA5 at a byte offset that rotates
through 0 .. 15 over the cases, the fragments and the old chunks are exactly as
long as the call may read and must not change.  The write runs in both
families, with each of the old arrays missing, and in place in the fragments of
the whole file, where every byte outside the window must stay.  One geometry
per bucket (k = 3, 7, 11 on n = 31) runs again with the fragments and the old
chunks 1 byte into their allocations.
"""
import numpy as np
import pytest

import _range_sweep as W
import _writev_rmw_cases as X
import test_gpu_readv_decode as TR
import test_gpu_writev_rmw as TW

pytestmark = pytest.mark.gpu

GEOM_MASKS = [(g, m) for g in W.GEOMS for m in range(3)]
GEOM_MASK_IDS = ["%s-mask%d" % (W.geom_id(g), m) for g, m in GEOM_MASKS]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def table(geom, m):
    """The cases of a (geometry, mask): the offsets go on where the last left."""
    return W.cases(geom, len(W.RANGES[geom]) * m + 5 * W.GEOMS.index(geom))


@pytest.mark.parametrize("geom,m", GEOM_MASKS, ids=GEOM_MASK_IDS)
def test_readv_decode_sweep_device(ec, oracle, geom, m):
    k, n = geom
    TR.run_cases(ec, W.oracle_for(oracle, k, n), k, n, W.masks(k, n)[m], table(geom, m))


@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("geom,m", GEOM_MASKS, ids=GEOM_MASK_IDS)
def test_writev_rmw_sweep_device(ec, oracle, geom, m, family):
    k, n = geom
    TW.run_cases(ec, W.oracle_for(oracle, k, n), k, n, W.masks(k, n)[m], table(geom, m), family)


@pytest.mark.parametrize("drop", W.DROPS, ids=lambda d: "no-" + "-".join(d))
@pytest.mark.parametrize("geom", W.GEOMS, ids=W.geom_id)
def test_writev_rmw_sweep_device_missing_old_stripes(ec, oracle, geom, drop):
    k, n = geom
    m = W.DROPS.index(drop)
    # with both arrays NULL the mask is ignored
    TW.run_cases(ec, W.oracle_for(oracle, k, n), k, n, W.masks(k, n)[m], table(geom, m),
                 "arbitrary", drop, given=0 if len(drop) == 2 else None)


@pytest.mark.parametrize("geom", W.offset_geoms(), ids=W.geom_id)
def test_readv_decode_sweep_device_fragments_off_alignment(ec, oracle, geom):
    k, n = geom
    TR.run_cases(ec, oracle, k, n, W.masks(k, n)[1], table(geom, 1), frag_offset=1)


@pytest.mark.parametrize("geom", W.offset_geoms(), ids=W.geom_id)
def test_writev_rmw_sweep_device_old_chunks_off_alignment(ec, oracle, geom):
    k, n = geom
    TW.run_cases(ec, oracle, k, n, W.masks(k, n)[1], table(geom, 1), "arbitrary", old_offset=1)


@pytest.mark.parametrize("geom", W.GEOMS, ids=W.geom_id)
def test_writev_rmw_sweep_device_in_place(ec, oracle, geom):
    """The fragments of the whole file are on the device, out[b] points into
    them at chunk `win` and the old chunks are the very chunks the call
    replaces: afterwards the fragments are those of the modified file, inside
    the window and outside it."""
    import torch
    k, n = geom
    O = W.oracle_for(oracle, k, n)
    mask = W.masks(k, n)[W.GEOMS.index(geom) % 3]
    bricks = [r - 1 for r in oracle.mask_rows(mask)]
    held = []
    for i, (head, size) in enumerate(W.RANGES[geom]):
        win = W.window(k, head, size, i)
        last = win + W.stripes(k, head, size) - 1
        user, frags, after = X.in_place(O, k, n, mask, head, size, win, i)
        dfrags = [TW.dev(f, (i + b) % 16) for b, f in enumerate(frags)]
        out = [f[win * W.CHUNK:] for f in dfrags]
        old_head = [dfrags[b][win * W.CHUNK:(win + 1) * W.CHUNK] for b in bricks]
        old_tail = [dfrags[b][last * W.CHUNK:(last + 1) * W.CHUNK] for b in bricks]
        assert old_head[0].data_ptr() == out[bricks[0]].data_ptr()
        held.append((head, size, TW.dev(user, i % 16), old_head, old_tail, out, dfrags, after))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        for head, size, user, old_head, old_tail, out, dfrags, after in held:
            assert L.writev_rmw_device(0, st.cuda_stream, head, size, user, mask, old_head,
                                       old_tail, out) == 0
        ec.sync_device(0, st.cuda_stream)
    for head, size, user, old_head, old_tail, out, dfrags, after in held:
        for b, (f, w) in enumerate(zip(dfrags, after)):
            assert np.array_equal(f.cpu().numpy(), w), \
                "%d+%d mask %#x range (%d, %d): fragment %d" % (k, n - k, mask, head, size, b)
