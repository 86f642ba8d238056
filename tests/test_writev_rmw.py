"""ec_method_writev_rmw on host buffers: the write of an unaligned byte range
over stored fragments, over the whole table of tests/_writev_rmw_cases.py.  No
GPU is needed: the host variant runs on the calling thread's CPU engine for
every gen.

The expected fragments are the oracle's encode of the window with the user
bytes in it.  Each case runs with one segment and with the user bytes cut at
two places into three segments of odd lengths, with an empty segment between
them.  Every output lies between 64 guard bytes of 0xA5 on each side, the old
chunks are arrays of exactly 512 bytes that may not change, and the engine
counters stay as they were.
"""
import ctypes
import errno

import numpy as np
import pytest

import _writev_rmw_cases as C

GENS = ["none", "avx"]
GUARD = 64


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def outputs(n, ns):
    """One buffer per fragment, each between two guards: (buffers, views)."""
    bufs = [np.full(GUARD + ns * C.CHUNK + GUARD, C.FILL, np.uint8) for _ in range(n)]
    return bufs, [b[GUARD:GUARD + ns * C.CHUNK] for b in bufs]


def check_outputs(bufs, ns, want, what):
    for i, (b, w) in enumerate(zip(bufs, want)):
        assert (b[:GUARD] == C.FILL).all() and (b[GUARD + ns * C.CHUNK:] == C.FILL).all(), \
            "%s: a guard of fragment %d was written" % (what, i)
        assert np.array_equal(b[GUARD:GUARD + ns * C.CHUNK], w), \
            "%s: fragment %d differs" % (what, i)


def split(user, k, head):
    c1, c2 = C.cuts(k, head, user.size)
    return [user[:c1].copy(), user[:0].copy(), user[c1:c2].copy(), user[c2:].copy()]


def run_case(L, k, n, head, mask, c, what):
    ns = C.stripes(k, head, c.user.size)
    olds = [a for a in (c.old_head, c.old_tail) if a is not None]
    copies = [[x.copy() for x in a] for a in olds]
    assert all(x.nbytes == C.CHUNK for a in olds for x in a)
    for user in (c.user, split(c.user, k, head)):
        bufs, views = outputs(n, ns)
        assert L.writev_rmw(head, user, mask, c.old_head, c.old_tail, views) == 0
        check_outputs(bufs, ns, c.want, what)
    for a, b in zip(olds, copies):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), what + ": an old chunk was written"


def test_table_covers_the_clip_ends():
    """What the table promises: every clip end on each residue mod 4, on a
    plane boundary +- 1 and on a chunk boundary +- 1; cuts that lie inside the
    write; every number of edges with and without an interior; 45 stripes at
    the most."""
    for k, _ in C.GEOMS:
        los, his = set(), set()
        for head, size in C.ranges(k):
            for lo, hi in C.clips(k, head, size):
                los.add(lo)
                his.add(hi)
            c1, c2 = C.cuts(k, head, size)
            assert 0 <= c1 <= c2 <= size
        for ends in (los, his):
            assert {e % 4 for e in ends} == {0, 1, 2, 3}
            assert {63, 64, 65, 511, 512, 513} <= ends
        # every number of edges, and the interior with and without them
        kinds = {(len(C.clips(k, h, s)), C.interior(k, h, s)[1] > 0) for h, s in C.ranges(k)}
        assert kinds == {(0, True), (1, False), (1, True), (2, False), (2, True)}
        assert max(C.stripes(k, h, s) for h, s in C.ranges(k)) <= 45


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%d+%d" % (g[0], g[1] - g[0]))
def test_writev_rmw_matches_oracle(ec, oracle, geom, family, gen):
    k, n = geom
    before = ec.stats()
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        i = 0
        for mask in C.masks(k, n):
            for head, size in C.ranges(k):
                what = "%d+%d mask %#x range (%d, %d) %s" % (k, n - k, mask, head, size, family)
                c = C.case(oracle, k, n, mask, head, size, C.window(k, head, size, i), i, family)
                i += 1
                run_case(L, k, n, head, mask, c, what)
    assert ec.stats() == before


@pytest.mark.parametrize("drop", C.DROPS, ids=lambda d: "no-" + "-".join(d))
@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%d+%d" % (g[0], g[1] - g[0]))
def test_missing_old_stripes_read_as_zeros(ec, oracle, geom, drop):
    k, n = geom
    with ec.ECMatrixList(k, n, gen="none") as L:
        for m, mask in enumerate(C.masks(k, n)):
            # with both arrays NULL the mask is ignored
            given = mask if len(drop) < 2 else (0, 1 << 40, mask)[m]
            for i, (head, size) in enumerate(C.ranges(k)):
                what = "%d+%d mask %#x range (%d, %d) without %s" % (k, n - k, mask, head, size,
                                                                    drop)
                c = C.case(oracle, k, n, mask, head, size, C.window(k, head, size, i), i,
                           "arbitrary", drop)
                run_case(L, k, n, head, given, c, what)


@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%d+%d" % (g[0], g[1] - g[0]))
def test_equals_writev_encode_of_the_decoded_stripes(ec, oracle, geom):
    k, n = geom
    mask = C.masks(k, n)[2]
    with ec.ECMatrixList(k, n, gen="none") as L:
        for i, (head, size) in enumerate(C.ranges(k)):
            for drop in [()] + C.DROPS:
                c = C.case(oracle, k, n, mask, head, size, 1, i, "arbitrary", drop)
                o0, o1 = C.decoded_olds(oracle, k, mask, c)
                ns = C.stripes(k, head, size)
                got = [np.full(ns * C.CHUNK, C.FILL, np.uint8) for _ in range(n)]
                ref = [np.full(ns * C.CHUNK, C.FILL, np.uint8) for _ in range(n)]
                assert L.writev_rmw(head, c.user, mask, c.old_head, c.old_tail, got) == 0
                assert L.writev_encode(head, c.user, o0, o1, ref) == 0
                for g, r, w in zip(got, ref, c.want):
                    assert np.array_equal(g, r) and np.array_equal(g, w), (head, size, drop)


@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%d+%d" % (g[0], g[1] - g[0]))
def test_aligned_ranges_equal_encode(ec, oracle, geom):
    k, n = geom
    S = C.CHUNK * k
    with ec.ECMatrixList(k, n, gen="none") as L:
        for nst in (1, 3):
            c = C.case(oracle, k, n, C.masks(k, n)[0], 0, nst * S)
            got = [np.full(nst * C.CHUNK, C.FILL, np.uint8) for _ in range(n)]
            ref = [np.full(nst * C.CHUNK, C.FILL, np.uint8) for _ in range(n)]
            # no old chunk is read: one byte each would do
            tiny = [np.zeros(1, np.uint8) for _ in range(k)]
            assert L.writev_rmw(0, c.user, C.masks(k, n)[0], tiny, tiny, got) == 0
            L.encode_batch(nst, c.user, ref)
            for g, r, w in zip(got, ref, c.want):
                assert np.array_equal(g, r) and np.array_equal(g, w)


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%d+%d" % (g[0], g[1] - g[0]))
def test_in_place(ec, oracle, geom, gen):
    """out[b] points into the fragments of the whole file at chunk `win` and
    the old chunks are the very chunks the call replaces."""
    k, n = geom
    with ec.ECMatrixList(k, n, gen=gen) as L:
        for m, mask in enumerate(C.masks(k, n)):
            bricks = [r - 1 for r in oracle.mask_rows(mask)]
            for i, (head, size) in enumerate(C.ranges(k)):
                win = C.window(k, head, size, i + m)
                ns = C.stripes(k, head, size)
                user, frags, after = C.in_place(oracle, k, n, mask, head, size, win, i)
                last = win + ns - 1
                out = [f[win * C.CHUNK:] for f in frags]
                old_head = [frags[b][win * C.CHUNK:(win + 1) * C.CHUNK] for b in bricks]
                old_tail = [frags[b][last * C.CHUNK:(last + 1) * C.CHUNK] for b in bricks]
                assert old_head[0].ctypes.data == out[bricks[0]].ctypes.data
                assert L.writev_rmw(head, user, mask, old_head, old_tail, out) == 0
                for b, (f, w) in enumerate(zip(frags, after)):
                    assert np.array_equal(f, w), \
                        "%d+%d mask %#x range (%d, %d): fragment %d" % (k, n - k, mask, head,
                                                                        size, b)


@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%d+%d" % (g[0], g[1] - g[0]))
def test_more_segments_than_the_stack_holds(ec, oracle, geom):
    """70 segments, every third one empty: the segment table of the call is on
    the heap from 65 segments on."""
    k, n = geom
    mask = C.masks(k, n)[2]
    head, size = 100, 5 * C.CHUNK * k + 33
    c = C.case(oracle, k, n, mask, head, size, 2, 3, "arbitrary")
    lengths = [0 if s % 3 == 1 else 2 * s + 1 for s in range(69)]
    lengths.append(size - sum(lengths))
    assert len(lengths) == 70 and lengths[-1] > 0
    ends = np.cumsum(lengths)
    user = [c.user[e - n_:e].copy() for e, n_ in zip(ends, lengths)]
    with ec.ECMatrixList(k, n, gen="none") as L:
        bufs, views = outputs(n, C.stripes(k, head, size))
        assert L.writev_rmw(head, user, mask, c.old_head, c.old_tail, views) == 0
        check_outputs(bufs, C.stripes(k, head, size), c.want, "70 segments")


def test_empty_write_writes_nothing(ec, oracle):
    k, n, mask = 4, 6, 0x3C
    c = C.case(oracle, k, n, mask, 5, 1)
    with ec.ECMatrixList(k, n, gen="none") as L:
        bufs, views = outputs(n, 1)
        empty = np.empty(0, np.uint8)
        assert L.writev_rmw(5, [empty, empty], mask, c.old_head, c.old_tail, views) == 0
        assert L.writev_rmw(5, [], mask, c.old_head, c.old_tail, views) == 0
        assert all((b == C.FILL).all() for b in bufs)
        # the argument checks come first
        with pytest.raises(OSError) as e:
            L.writev_rmw(C.CHUNK * k, [empty], mask, c.old_head, c.old_tail, views)
        assert e.value.errno == errno.EINVAL


# ---- every -EINVAL of the contract

def raw(ec, a):
    return ec.lib.ec_method_writev_rmw(a["L"], a["head"], a["iov"], a["count"], a["mask"],
                                       a["old_head"], a["old_tail"], a["out"])


@pytest.fixture()
def call(ec, oracle):
    """A valid call of 4+2, mask 0x3C, range (100, 3000), as a dict of the raw
    arguments, with what keeps them alive."""
    k, n, mask, head, size = 4, 6, 0x3C, 100, 3000
    c = C.case(oracle, k, n, mask, head, size)
    ns = C.stripes(k, head, size)
    out = [np.full(ns * C.CHUNK, C.FILL, np.uint8) for _ in range(n)]
    with ec.ECMatrixList(k, n, gen="none") as L:
        iov = (ec._IOVec * 1)(ec._IOVec(c.user.ctypes.data, size))
        yield dict(L=ctypes.byref(L._list), head=head, iov=iov, count=1, mask=mask,
                   old_head=ec._ptr_array(c.old_head), old_tail=ec._ptr_array(c.old_tail),
                   out=ec._ptr_array(out), keep=(c, out))
        # no rejected call wrote a byte
        assert all((o == C.FILL).all() for o in out)


def rejected(ec, call, text, **changed):
    rc = raw(ec, dict(call, **changed))
    assert rc == -errno.EINVAL
    err = ec.lib.ec_method_last_error().decode()
    assert err.startswith("ec_method_writev_rmw: ") and text in err, err


def test_the_valid_call_of_the_error_tests(ec, call):
    c, out = call["keep"]
    assert raw(ec, call) == 0
    for o, w in zip(out, c.want):
        assert np.array_equal(o, w)
        o[:] = C.FILL


def test_einval_null_list(ec, call):
    rejected(ec, call, "list", L=None)


def test_einval_null_out(ec, call):
    rejected(ec, call, "output list", out=None)


def test_einval_null_output(ec, call):
    out = call["keep"][1]
    for i in range(6):
        given = list(out)
        given[i] = None
        rejected(ec, call, "output is NULL", out=ec._ptr_array(given))


def test_einval_null_iov(ec, call):
    rejected(ec, call, "segment list", iov=None)


def test_einval_negative_count(ec, call):
    rejected(ec, call, "count", count=-1)


def test_einval_null_segment_with_length(ec, call):
    c, out = call["keep"]
    iov = (ec._IOVec * 2)(ec._IOVec(c.user.ctypes.data, 10), ec._IOVec(None, 5))
    rejected(ec, call, "segment is NULL", iov=iov, count=2)
    # with length 0 a NULL base is a segment like any other
    iov = (ec._IOVec * 2)(ec._IOVec(None, 0), ec._IOVec(c.user.ctypes.data, 3000))
    assert raw(ec, dict(call, iov=iov, count=2)) == 0
    for o, w in zip(out, c.want):
        assert np.array_equal(o, w)
        o[:] = C.FILL


def test_einval_head_outside_first_stripe(ec, call):
    rejected(ec, call, "head", head=4 * C.CHUNK)
    rejected(ec, call, "head", head=1 << 40)


def test_einval_mask(ec, call):
    for mask in (0, 0x1C, 0x3E, 0x4E, 0x10F, (1 << 20) - 1):
        rejected(ec, call, "mask", mask=mask)
        rejected(ec, call, "mask", mask=mask, old_head=None)
        rejected(ec, call, "mask", mask=mask, old_tail=None)


def test_einval_null_old_chunk(ec, call):
    c = call["keep"][0]
    for which, chunks in (("old_head", c.old_head), ("old_tail", c.old_tail)):
        for p in range(4):
            given = list(chunks)
            given[p] = None
            rejected(ec, call, "old chunk is NULL", **{which: ec._ptr_array(given)})


def test_einval_device_entry_with_host_buffers(ec, call):
    """Host buffers given to the device entry point: -EINVAL with a device,
    and never a write."""
    c = call["keep"][0]
    rc = ec.lib.ec_method_writev_rmw_device(call["L"], 0, None, call["head"], c.user.size,
                                            c.user.ctypes.data, call["mask"], call["old_head"],
                                            call["old_tail"], call["out"])
    assert rc == -errno.EINVAL
