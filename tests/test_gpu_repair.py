"""ec_method_repair_device: rewrite the chunks loc[] names on device-resident
fragments (ec_repair_n, ec_kernels_impl.h).  The geometries, sizes and cases
of tests/test_repair.py on torch device tensors, with expected bytes from the
oracle (tests/_repair_cases.py), plus what only the kernel can get wrong: 1027
stripes (several blocks, a ragged last wave) with every stripe dirty and the
bricks taking turns inside one wave's 64 words, every stripe naming one brick
(groups of four), a dirty stripe in lane 63 beside one in lane 0 of the next
wave, 16+15, fragments at odd byte addresses including the one written, a
caller's stream with locate -> repair -> locate queued back to back, and 2^15
stripes.  Every fragment is followed by a guard chunk that must not change.
"""
import errno

import numpy as np
import pytest

import _repair_cases as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = R.CHUNK


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def dev(a, offset=0):
    """A device copy of numpy array `a`, starting `offset` bytes into its
    allocation."""
    import torch
    t = torch.empty(a.nbytes + offset, dtype=torch.uint8, device=DEV)
    v = t[offset:]
    v.copy_(torch.from_numpy(np.array(a, dtype=np.uint8)))    # (a may be read-only)
    return v


class DeviceOps:
    """Every call uploads its fragments, guard chunk included, and reads all
    of them back after one synchronisation."""

    def __init__(self, ec, L, nst, avail_mask, stream=None, offsets=None):
        self.ec, self.L, self.nst, self.mask = ec, L, nst, avail_mask
        self.stream, self.offs = stream, offsets or {}

    def _upload(self, frags):
        full = [None if f is None else dev(R.with_guard(f), self.offs.get(b, 0))
                for b, f in enumerate(frags)]
        return full, [None if f is None else f[:self.nst * CHUNK] for f in full]

    def _loc(self, fill=None):
        import torch
        if fill is None:
            return torch.full((self.nst,), -1, dtype=torch.int32, device=DEV)
        return torch.from_numpy(fill.view(np.int32).copy()).to(DEV)

    @staticmethod
    def _host(full):
        return [None if f is None else f.cpu().numpy() for f in full]

    def repair(self, frags, loc):
        import torch
        full, view = self._upload(frags)
        dloc = self._loc(loc)
        torch.cuda.synchronize()
        self.L.repair_device(0, self.stream, self.nst, self.mask, view, dloc)
        self.ec.sync_device(0, self.stream)
        return self._host(full), dloc.cpu().numpy().view(np.uint32), None

    def scrub(self, frags):
        import torch
        full, view = self._upload(frags)
        loc, loc2 = self._loc(), self._loc()
        torch.cuda.synchronize()
        # queued back to back: no host synchronisation between the three
        self.L.locate_device(0, self.stream, self.nst, self.mask, view, loc)
        self.L.repair_device(0, self.stream, self.nst, self.mask, view, loc)
        self.L.locate_device(0, self.stream, self.nst, self.mask, view, loc2)
        self.ec.sync_device(0, self.stream)
        return (loc.cpu().numpy().view(np.uint32), self._host(full),
                loc2.cpu().numpy().view(np.uint32), None)


@pytest.mark.parametrize("nst", R.SIZES + [1027])
@pytest.mark.parametrize("geom", R.GEOMS + [R.GEOM_LARGEST], ids=R.geom_id)
def test_repair_device_matches_oracle(ec, oracle, geom, nst):
    k, n, avail_mask = geom
    with ec.ECMatrixList(k, n) as L:
        R.run_geometry(DeviceOps(ec, L, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_repair_device_fragments_at_odd_addresses(ec, oracle):
    """Every fragment 1 byte into its allocation (4+2), and a mix of byte
    offsets 1, 0, 3, 2 over the bricks (8+4): inputs and the written fragment
    at byte addresses."""
    k, n, avail_mask, nst = 4, 6, 0x3F, 67
    with ec.ECMatrixList(k, n) as L:
        R.run_geometry(DeviceOps(ec, L, nst, avail_mask, offsets={b: 1 for b in range(n)}),
                       oracle, k, n, avail_mask, nst)
    k, n, avail_mask, nst = 8, 12, 0xF6F, 5
    with ec.ECMatrixList(k, n) as L:
        offs = {b: (1, 0, 3, 2)[j % 4] for j, b in enumerate(R.bits(avail_mask))}
        R.run_geometry(DeviceOps(ec, L, nst, avail_mask, offsets=offs), oracle, k, n,
                       avail_mask, nst)


def test_repair_device_on_a_callers_stream(ec, oracle):
    """locate -> repair -> locate on a caller's stream, one sync at the end."""
    import torch
    k, n, avail_mask, nst = 8, 12, 0xF6F, 67
    st = torch.cuda.Stream()
    with ec.ECMatrixList(k, n) as L:
        R.run_geometry(DeviceOps(ec, L, nst, avail_mask, stream=st.cuda_stream), oracle, k, n,
                       avail_mask, nst)


def test_repair_device_at_scale(ec, oracle):
    """8+4 with all 12 bricks, 2^15 stripes, 97 seeded single-bit flips in
    distinct stripes spread over all 12 bricks: locate, repair, and every
    fragment equals the oracle's clean one over all entries."""
    import torch
    k, n, avail_mask, nst = 8, 12, 0xFFF, 1 << 15
    frags = R.fragments(oracle, k, n, nst)
    full = [dev(R.with_guard(f)) for f in frags]
    dfr = [f[:nst * CHUNK] for f in full]
    rng = np.random.default_rng(97)
    stripes = rng.choice(nst, size=97, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    want = np.zeros(nst, np.uint32)
    for j, t in enumerate(stripes.tolist()):
        b = j % n
        off = t * CHUNK + int(rng.integers(0, CHUNK))
        dfr[b][off] ^= 1 << int(rng.integers(0, 8))
        want[t] = 1 << b
    loc = torch.full((nst,), -1, dtype=torch.int32, device=DEV)
    loc2 = torch.full((nst,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.locate_device(0, None, nst, avail_mask, dfr, loc)
        L.repair_device(0, None, nst, avail_mask, dfr, loc)
        L.locate_device(0, None, nst, avail_mask, dfr, loc2)
        ec.sync_device(0)
    assert np.array_equal(loc.cpu().numpy().view(np.uint32), want)
    assert not loc2.cpu().numpy().any()
    try:
        R.check_frags("at scale", list(range(n)), nst, [f.cpu().numpy() for f in full], frags)
    finally:
        from _locate_cases import _frag_cache
        _frag_cache.pop((k, n, nst), None)      # 192 MiB: not kept for the session


def test_repair_rejects_mixed_host_and_device_buffers(ec, oracle):
    """Device tensors given to the host entry point, host arrays to the device
    entry point, all of them or mixed: -EINVAL, nothing written."""
    import torch
    k, n, nst = 4, 6, 4
    clean = R.fragments(oracle, k, n, nst)
    frags = [R.flipped(f, 1, 9, 1) for f in clean]
    keep = [f.copy() for f in frags]
    dfr = [dev(f) for f in frags]
    hloc = np.full(nst, 1 << 1, np.uint32)
    dloc = torch.from_numpy(hloc.view(np.int32).copy()).to(DEV)
    with ec.ECMatrixList(k, n) as L:
        for fr, loc in (
                (dfr, dloc),                                   # all on the device
                (dfr, hloc),
                ([frags[0], dfr[1]] + frags[2:], hloc),        # the named brick
                (frags[:5] + [dfr[5]], hloc),                  # a brick that is not read
                (frags, dloc)):
            with pytest.raises(OSError) as e:
                L.repair(nst, 0x3F, fr, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_repair" in str(e.value)
        for fr, loc in (
                ([dfr[0], frags[1]] + dfr[2:], dloc),
                (dfr[:5] + [frags[5]], dloc),
                (dfr, hloc)):
            with pytest.raises(OSError) as e:
                L.repair_device(0, None, nst, 0x3F, fr, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_repair_device" in str(e.value)
        ec.sync_device(0)
    for b in range(n):
        assert np.array_equal(frags[b], keep[b])
        assert np.array_equal(dfr[b].cpu().numpy(), keep[b])
    assert (hloc == 1 << 1).all()
    assert (dloc.cpu().numpy().view(np.uint32) == 1 << 1).all()
