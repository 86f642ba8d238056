"""ec_method_writev_rmw_device: the write of an unaligned byte range over stored
fragments in device memory, over the whole table of
tests/_writev_rmw_cases.py: every K bucket of the edge kernel ec_rmw_edge (with
the run-time k below the bucket), writes inside one stripe, over two stripes
with no interior, and with interior stripes for the encoder, whose input then
starts head bytes behind a stripe boundary.

The expected fragments are the oracle's encode of the window with the user
bytes in it, never the library's.  Each out[i] is carved from a tensor with
2 KiB of 0xA5 on each side, which must stay as they are, at a byte offset that
rotates through 0 .. 15 over the cases, and `user` sits at a rotating offset
too; the old-chunk tensors are exactly 512 bytes and may not change.  One
geometry per bucket runs the cases (65, 3) and (100, 5 S + 33) at all 16
output offsets and the whole table again with every old chunk 1 byte into its
allocation.  The calls of one mask are queued on one side stream with one
sync.
"""
import errno

import numpy as np
import pytest

import _writev_rmw_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 2048


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


def dev_chunks(chunks, offset=0):
    return None if chunks is None else [dev(c, offset) for c in chunks]


def new_outs(n, ns, offset):
    """(the whole tensors, the outputs): ns chunks between two guards of 0xA5,
    each output `offset` bytes past a 16-byte boundary."""
    import torch
    size = ns * C.CHUNK
    ts = [torch.full((GUARD + offset + size + GUARD,), C.FILL, dtype=torch.uint8, device=DEV)
          for _ in range(n)]
    assert all(t.data_ptr() % 16 == 0 for t in ts)
    return ts, [t[GUARD + offset:GUARD + offset + size] for t in ts]


def check_outs(ts, ns, offset, want, what):
    lo, size = GUARD + offset, ns * C.CHUNK
    for i, (t, w) in enumerate(zip(ts, want)):
        got = t.cpu().numpy()
        assert (got[:lo] == C.FILL).all(), "%s: bytes in front of out[%d] were written" % (what, i)
        assert (got[lo + size:] == C.FILL).all(), \
            "%s: bytes behind out[%d] were written" % (what, i)
        assert np.array_equal(got[lo:lo + size], w), "%s: out[%d] differs" % (what, i)


def run_cases(ec, oracle, k, n, mask, cases, family="file", drop=(), old_offset=0, given=None):
    """cases: (head, size, out offset).  All queued on one side stream, then
    one sync and the checks."""
    import torch
    held = []
    for i, (head, size, off) in enumerate(cases):
        c = C.case(oracle, k, n, mask, head, size, C.window(k, head, size, i), i, family, drop)
        ns = C.stripes(k, head, size)
        olds = (dev_chunks(c.old_head, old_offset), dev_chunks(c.old_tail, old_offset))
        assert all(t.numel() == C.CHUNK for o in olds if o for t in o)
        held.append((head, size, off, c, ns, dev(c.user, (off * 7 + i) % 16), olds,
                     new_outs(n, ns, off)))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        for head, size, off, c, ns, user, (oh, ot), (ts, outs) in held:
            assert L.writev_rmw_device(0, st.cuda_stream, head, size, user,
                                       mask if given is None else given, oh, ot, outs) == 0
        ec.sync_device(0, st.cuda_stream)
    for head, size, off, c, ns, user, olds, (ts, outs) in held:
        what = "%d+%d mask %#x range (%d, %d) out + %d %s %s" % (k, n - k, mask, head, size, off,
                                                                 family, drop)
        check_outs(ts, ns, off, c.want, what)
        for have, was in zip(olds, (c.old_head, c.old_tail)):
            for d, h in zip(have or [], was or []):
                assert np.array_equal(d.cpu().numpy(), h), what + ": an old chunk was written"
        assert np.array_equal(user.cpu().numpy(), c.user), what + ": user was written"


GEOM_MASKS = [(k, n, m) for k, n in C.GEOMS for m in range(3)]
GEOM_MASK_IDS = ["%d+%d-mask%d" % (k, n - k, m) for k, n, m in GEOM_MASKS]


def table(k, n, m):
    ranges = C.ranges(k)
    first = len(ranges) * GEOM_MASKS.index((k, n, m))   # the offsets go on where the last left
    return [(head, size, (first + i) % 16) for i, (head, size) in enumerate(ranges)]


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("k,n,m", GEOM_MASKS, ids=GEOM_MASK_IDS)
def test_writev_rmw_device_matches_oracle(ec, oracle, k, n, m, family):
    run_cases(ec, oracle, k, n, C.masks(k, n)[m], table(k, n, m), family)


@pytest.mark.parametrize("drop", C.DROPS, ids=lambda d: "no-" + "-".join(d))
@pytest.mark.parametrize("k,n", C.GEOMS, ids=lambda v: str(v))
def test_missing_old_stripes_read_as_zeros(ec, oracle, k, n, drop):
    m = C.DROPS.index(drop)
    # with both arrays NULL the mask is ignored
    run_cases(ec, oracle, k, n, C.masks(k, n)[m], table(k, n, m), "arbitrary", drop,
              given=0 if len(drop) == 2 else None)


@pytest.mark.parametrize("k,n", C.BUCKET_GEOMS, ids=lambda v: str(v))
def test_writev_rmw_device_at_every_out_offset(ec, oracle, k, n):
    cases = [(head, size, off) for head, size in C.offset_ranges(k) for off in range(16)]
    run_cases(ec, oracle, k, n, C.masks(k, n)[2], cases, "arbitrary")


@pytest.mark.parametrize("k,n", C.BUCKET_GEOMS, ids=lambda v: str(v))
def test_writev_rmw_device_old_chunks_off_alignment(ec, oracle, k, n):
    cases = [(head, size, (5 + i) % 16) for i, (head, size) in enumerate(C.ranges(k))]
    run_cases(ec, oracle, k, n, C.masks(k, n)[1], cases, "arbitrary", old_offset=1)


@pytest.mark.parametrize("k,n,m", GEOM_MASKS, ids=GEOM_MASK_IDS)
def test_in_place(ec, oracle, k, n, m):
    """The fragments of the whole file are on the device, out[b] points into
    them at chunk `win` and the old chunks are the very chunks the call
    replaces: afterwards the fragments are those of the modified file, inside
    the window and outside it."""
    import torch
    mask = C.masks(k, n)[m]
    bricks = [r - 1 for r in oracle.mask_rows(mask)]
    held = []
    for i, (head, size) in enumerate(C.ranges(k)):
        win = C.window(k, head, size, i + m)
        last = win + C.stripes(k, head, size) - 1
        user, frags, after = C.in_place(oracle, k, n, mask, head, size, win, i)
        dfrags = [dev(f, (i + b) % 16) for b, f in enumerate(frags)]
        out = [f[win * C.CHUNK:] for f in dfrags]
        old_head = [dfrags[b][win * C.CHUNK:(win + 1) * C.CHUNK] for b in bricks]
        old_tail = [dfrags[b][last * C.CHUNK:(last + 1) * C.CHUNK] for b in bricks]
        assert old_head[0].data_ptr() == out[bricks[0]].data_ptr()
        held.append((head, size, dev(user, i % 16), old_head, old_tail, out, dfrags, after))
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


@pytest.mark.parametrize("k,n", C.GEOMS, ids=lambda v: str(v))
def test_aligned_ranges_equal_encode_device(ec, oracle, k, n):
    import torch
    S = C.CHUNK * k
    mask = C.masks(k, n)[0]
    with ec.ECMatrixList(k, n) as L:
        for nst in (1, 3):
            c = C.case(oracle, k, n, mask, 0, nst * S)
            user = dev(c.user)
            ts, outs = new_outs(n, nst, 0)
            ref = [torch.full((nst * C.CHUNK,), C.FILL, dtype=torch.uint8, device=DEV)
                   for _ in range(n)]
            # no old chunk is read: one byte each would do
            tiny = [torch.zeros(1, dtype=torch.uint8, device=DEV) for _ in range(k)]
            torch.cuda.synchronize()
            assert L.writev_rmw_device(0, None, 0, nst * S, user, mask, tiny, tiny, outs) == 0
            L.encode_device(0, None, nst, user, ref)
            ec.sync_device(0)
            check_outs(ts, nst, 0, c.want, "aligned")
            assert all(torch.equal(o, r) for o, r in zip(outs, ref))


@pytest.mark.parametrize("k,n", C.GEOMS, ids=lambda v: str(v))
def test_agrees_with_writev_encode_device_fed_by_decode_device(ec, oracle, k, n):
    """The parent's route: decode_device of each edge stripe into a temporary,
    then writev_encode_device."""
    import torch
    S = C.CHUNK * k
    mask = C.masks(k, n)[2]
    with ec.ECMatrixList(k, n) as L:
        for i, (head, size) in enumerate(C.ranges(k)):
            c = C.case(oracle, k, n, mask, head, size, 1, i, "arbitrary")
            ns = C.stripes(k, head, size)
            user = dev(c.user)
            oh, ot = dev_chunks(c.old_head), dev_chunks(c.old_tail)
            o0 = torch.empty(S, dtype=torch.uint8, device=DEV)
            o1 = torch.empty(S, dtype=torch.uint8, device=DEV)
            ts, outs = new_outs(n, ns, 0)
            ref = [torch.full((ns * C.CHUNK,), C.FILL, dtype=torch.uint8, device=DEV)
                   for _ in range(n)]
            torch.cuda.synchronize()
            assert L.writev_rmw_device(0, None, head, size, user, mask, oh, ot, outs) == 0
            L.decode_device(0, None, 1, mask, oh, o0)
            L.decode_device(0, None, 1, mask, ot, o1)
            L.writev_encode_device(0, None, head, size, user, o0, o1, ref)
            ec.sync_device(0)
            for o, r, w in zip(outs, ref, c.want):
                assert torch.equal(o, r), (head, size)
                assert np.array_equal(o.cpu().numpy(), w), (head, size)


def test_readv_decode_device_follows_the_write_on_the_stream(ec, oracle):
    """writev_rmw_device in place, then readv_decode_device of the written
    range, on one stream with no synchronisation between them."""
    import torch
    k, n, mask = 4, 6, 0x3C
    bricks = [r - 1 for r in oracle.mask_rows(mask)]
    st = torch.cuda.Stream()
    with ec.ECMatrixList(k, n) as L:
        for i, (head, size) in enumerate([(100, 5 * C.CHUNK * k + 33), (65, 3), (0, 1),
                                          (7, 2 * C.CHUNK * k)]):
            win = 2
            last = win + C.stripes(k, head, size) - 1
            user, frags, after = C.in_place(oracle, k, n, mask, head, size, win, i)
            dfrags = [dev(f) for f in frags]
            duser = dev(user, 3)
            back = torch.full((GUARD + size + GUARD,), C.FILL, dtype=torch.uint8, device=DEV)
            out = [f[win * C.CHUNK:] for f in dfrags]
            old_head = [dfrags[b][win * C.CHUNK:(win + 1) * C.CHUNK] for b in bricks]
            old_tail = [dfrags[b][last * C.CHUNK:(last + 1) * C.CHUNK] for b in bricks]
            torch.cuda.synchronize()
            L.writev_rmw_device(0, st.cuda_stream, head, size, duser, mask, old_head, old_tail,
                                out)
            L.readv_decode_device(0, st.cuda_stream, head, size, mask, [out[b] for b in bricks],
                                  back[GUARD:GUARD + size])
            ec.sync_device(0, st.cuda_stream)
            got = back.cpu().numpy()
            assert np.array_equal(got[GUARD:GUARD + size], user), (head, size)
            assert (got[:GUARD] == C.FILL).all() and (got[GUARD + size:] == C.FILL).all()


def test_empty_write_on_device(ec, oracle):
    k, n, mask = 4, 6, 0x3C
    c = C.case(oracle, k, n, mask, 5, 1)
    oh, ot = dev_chunks(c.old_head), dev_chunks(c.old_tail)
    ts, outs = new_outs(n, 1, 0)
    with ec.ECMatrixList(k, n) as L:
        assert L.writev_rmw_device(0, None, 5, 0, dev(c.user), mask, oh, ot, outs) == 0
        assert L.writev_rmw_device(0, None, 5, 0, None, mask, oh, ot, outs) == 0
        # the argument checks come first
        with pytest.raises(OSError) as e:
            L.writev_rmw_device(0, None, C.CHUNK * k, 0, None, mask, oh, ot, outs)
        assert e.value.errno == errno.EINVAL
        ec.sync_device(0)
    assert all((t.cpu().numpy() == C.FILL).all() for t in ts)


def test_writev_rmw_device_argument_errors(ec, oracle):
    k, n, mask, head, size = 4, 6, 0x3C, 100, 3000
    c = C.case(oracle, k, n, mask, head, size)
    ns = C.stripes(k, head, size)
    user = dev(c.user, 1)
    oh, ot = dev_chunks(c.old_head), dev_chunks(c.old_tail)
    ts, outs = new_outs(n, ns, 1)
    houts = [np.full(ns * C.CHUNK, C.FILL, np.uint8) for _ in range(n)]

    def rejected(call, *args):
        with pytest.raises(OSError) as e:
            call(*args)
        assert e.value.errno == errno.EINVAL, e.value

    with ec.ECMatrixList(k, n) as L:
        d = L.writev_rmw_device
        # host pointers given to the device entry point, all or some
        rejected(d, 0, None, head, size, c.user, mask, c.old_head, c.old_tail, houts)
        rejected(d, 0, None, head, size, c.user, mask, oh, ot, outs)
        rejected(d, 0, None, head, size, user, mask, c.old_head, ot, outs)
        rejected(d, 0, None, head, size, user, mask, oh, ot[:3] + c.old_tail[3:], outs)
        rejected(d, 0, None, head, size, user, mask, oh, ot, outs[:5] + houts[5:])
        # device pointers given to the host entry point, all or some
        rejected(L.writev_rmw, head, user, mask, oh, ot, outs)
        rejected(L.writev_rmw, head, user, mask, c.old_head, c.old_tail, houts)
        rejected(L.writev_rmw, head, c.user, mask, oh, c.old_tail, houts)
        rejected(L.writev_rmw, head, c.user, mask, c.old_head, c.old_tail, houts[:5] + outs[5:])
        # head outside the first stripe
        rejected(d, 0, None, C.CHUNK * k, size, user, mask, oh, ot, outs)
        # masks of k - 1 and k + 1 bricks, with a brick at n, and none
        for bad in (0x1C, 0x3E, 0x4E, 0):
            rejected(d, 0, None, head, size, user, bad, oh, ot, outs)
            rejected(d, 0, None, head, size, user, bad, None, ot, outs)
        rejected(d, 0, None, head, size, user, mask, oh[:3] + [None], ot, outs)
        rejected(d, 0, None, head, size, user, mask, oh, ot[:3] + [None], outs)
        rejected(d, 0, None, head, size, user, mask, oh, ot, outs[:5] + [None])
        rejected(d, 0, None, head, size, None, mask, oh, ot, outs)
        ec.sync_device(0)
        assert all((t.cpu().numpy() == C.FILL).all() for t in ts)
        assert all((h == C.FILL).all() for h in houts)
        # and the call they all fall short of
        assert d(0, None, head, size, user, mask, oh, ot, outs) == 0
        ec.sync_device(0)
    check_outs(ts, ns, 1, c.want, "valid")
