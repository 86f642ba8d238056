"""ec_method_heal_checked2_device over every brick, every pair of bricks and
every k from 2 to 16 (the geometries of tests/test_heal_checked2_sweep.py, the
case builder of tests/_scrub_sweep.py): ec_heal_checked2_n with the run-time k
at every value of each K bucket and every entry of the pair tables that travel
in its kernel arguments, then repair2 and a second locate2 queued behind it on
the same stream.

Nothing expected comes from the library: the rule of include/ec_method.h names
every damaged brick and pair, every target chunk is the chunk the data encodes
to, repair2 restores the clean fragments and the second locate2 is all zero.
"""
import numpy as np
import pytest

import _scrub_sweep as W
from test_heal_checked2_sweep import sweep_geoms, targets_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8)).to(DEV)    # (a may be read-only)


@pytest.mark.parametrize("geom", sweep_geoms(), ids=W.geom_id)
def test_heal_checked2_sweep_device(ec, oracle, geom):
    import torch
    S = W.built(geom)
    assert S.two
    k, n, nst, am = S.k, S.n, S.nst, S.avail_mask
    targets = targets_of(geom)
    filler = np.full(W.CHUNK * nst, 0x3C, np.uint8)
    dfr = [dev(filler if f is None else f) for f in S.frags]
    loc, again = (torch.full((nst + W.GUARD,), -1, dtype=torch.int32, device=DEV)
                  for _ in range(2))
    out = [torch.full((W.CHUNK * (nst + 1),), W.FILL, dtype=torch.uint8, device=DEV)
           for _ in targets]
    st = torch.cuda.Stream()
    s = st.cuda_stream
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.heal_checked2_device(0, s, nst, am, dfr, W.mask_of(targets), out, loc)
        ec.sync_device(0, s)
        for b, f in enumerate(S.frags):
            assert np.array_equal(dfr[b].cpu().numpy(), filler if f is None else f), \
                "the buffer of brick %d was written" % b
        # the same call again with repair2 and locate2 behind it, one sync
        L.heal_checked2_device(0, s, nst, am, dfr, W.mask_of(targets), out, loc)
        L.repair2_device(0, s, nst, am, dfr, loc)
        L.locate2_device(0, s, nst, am, dfr, again)
        ec.sync_device(0, s)
    got = loc.cpu().numpy().view(np.uint32)
    assert (got[nst:] == W.SENTINEL).all(), "guard words written"
    d = np.flatnonzero(got[:nst] != S.loc2)
    assert d.size == 0, [(t, S.cases[t], hex(got[t])) for t in d[:8]]
    for j, o in zip(targets, out):
        o = o.cpu().numpy()
        assert (o[W.CHUNK * nst:] == W.FILL).all(), "guard chunk written"
        d = np.flatnonzero((o[:W.CHUNK * nst].reshape(nst, W.CHUNK) !=
                            S.clean[j].reshape(nst, W.CHUNK)).any(axis=1))
        assert d.size == 0, (j, [(t, S.cases[t]) for t in d[:8]])
    assert not again.cpu().numpy()[:nst].any(), "locate2 after repair2"
    for b, f in enumerate(S.frags):
        want = filler if f is None else S.clean[b]
        assert np.array_equal(dfr[b].cpu().numpy(), want), "brick %d after repair2" % b
