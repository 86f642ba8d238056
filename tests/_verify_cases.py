"""Shared cases of tests/test_verify.py (host buffers, CPU engine) and
tests/test_gpu_verify.py (device buffers, ec_verify_n): geometries, masks,
corruptions and the expected flags of ec_method_verify[_device].

Expected values come from the oracle, never from the library: the chunk a
check brick i should hold is encode(k, n, decode(k, rows(mask), in))[i], and
bad[t] is the OR of 1 << i over the check bricks whose stored chunk t differs
from it.  The code is MDS, so every coefficient of the prediction matrix is
non-zero, which gives two rules asserted beside the oracle's result: a flipped
bit in a check brick sets exactly that brick's bit, a flipped bit in a basis
brick sets the bit of every check brick.
"""
import numpy as np

CHUNK = 512
GUARD = 8                       # words after bad[nstripes) that must not change
SENTINEL = 0xFFFFFFFF

# (k, n, mask, check_mask): a leading and a non-leading basis, one check brick
# alone and all n - k of them
GEOMS = [
    (2, 3, 0x3, 0x4),
    (2, 3, 0x6, 0x1),
    (4, 6, 0x0F, 0x30),
    (4, 6, 0x3C, 0x03),
    (4, 6, 0x0F, 0x20),
    (8, 12, 0x0FF, 0xF00),
    (8, 12, 0xD6B, 0x294),
    (8, 12, 0x0FF, 0x400),
    (16, 20, 0x0FFFF, 0xF0000),
    (16, 20, 0xFFFF0, 0x0000F),
    (16, 20, 0x0FFFF, 0x20000),
]
SIZES = [1, 3, 4, 5, 67]


def geom_id(g):
    return "%d+%d-%x-%x" % (g[0], g[1] - g[0], g[2], g[3])


def bits(mask):
    return [i for i in range(64) if (mask >> i) & 1]


_frag_cache = {}


def fragments(O, k, n, nst):
    """The n oracle-encoded fragments of nst stripes of random data (shared,
    read-only)."""
    key = (k, n, nst)
    if key not in _frag_cache:
        data = np.random.default_rng(1000 * k + 10 * n + nst).integers(
            0, 256, size=CHUNK * k * nst, dtype=np.uint8)
        frags = O.encode(k, n, data, nthreads=8 if nst > 4096 else 1)
        for f in frags:
            f.setflags(write=False)
        _frag_cache[key] = frags
    return _frag_cache[key]


def predict(O, k, n, mask, ins, stripes=None):
    """Oracle prediction of all n fragments from the k basis fragments `ins`
    (bricks of mask), for every stripe or for the listed ones only (stripes
    are independent); returns {stripe: [n chunks]} or the n whole fragments."""
    rows = [b + 1 for b in bits(mask)]
    if stripes is None:
        return O.encode(k, n, O.decode(k, rows, ins))
    out = {}
    for t in stripes:
        sl = [np.ascontiguousarray(f[t * CHUNK:(t + 1) * CHUNK]) for f in ins]
        out[t] = O.encode(k, n, O.decode(k, rows, sl))
    return out


def expected_flags(pred, check_mask, checks, nst):
    """bad[] from the predicted fragments `pred` (all n) and the stored ones."""
    bad = np.zeros(nst, np.uint32)
    for j, i in enumerate(bits(check_mask)):
        diff = (pred[i].reshape(nst, CHUNK) != checks[j].reshape(nst, CHUNK)).any(axis=1)
        bad |= diff.astype(np.uint32) << np.uint32(i)
    return bad


def single_flips(k, m, nst):
    """Eight single-bit flips, one per plane (plane b = bytes [64b, 64b + 64)
    of a chunk; flip j also flips bit j of its byte): the first byte of a
    chunk (plane 0) and the last (plane 7), stripe 0 and the last stripe, a
    basis brick and a check brick in every combination.
    (kind, position in in[] / check[], stripe, byte in chunk, bit)."""
    out = []
    for j in range(8):
        byte = 0 if j == 0 else 511 if j == 7 else 64 * j + (13 * j + 5) % 64
        assert byte // 64 == j
        kind = "check" if (j >> 1) & 1 else "basis"
        out.append((kind, j % (m if kind == "check" else k), 0 if j % 2 == 0 else nst - 1,
                    byte, j))
    return out


def flipped(buf, stripe, byte, bit):
    c = buf.copy()
    c[stripe * CHUNK + byte] ^= np.uint8(1 << bit)
    return c


def run_geometry(run, O, k, n, mask, check_mask, nst):
    """Every corruption case of one geometry and size.  run(ins, checks) ->
    (bad[0..nst) as uint32, nbad or None); the runner checks its own sentinel
    and guard words."""
    frags = fragments(O, k, n, nst)
    basis, cb = bits(mask), bits(check_mask)
    m = len(cb)
    ins = [frags[b] for b in basis]
    checks = [frags[b] for b in cb]
    pred = predict(O, k, n, mask, ins)

    def verify(ins_, checks_, want, what):
        bad, nbad = run(ins_, checks_)
        assert np.array_equal(bad, want), (what, np.flatnonzero(bad != want)[:8], bad[:8], want[:8])
        if nbad is not None:
            assert nbad == int(np.count_nonzero(want)), (what, nbad)

    # clean fragments: all-zero flags
    want = expected_flags(pred, check_mask, checks, nst)
    assert not want.any()
    verify(ins, checks, want, "clean")

    for kind, pos, t, byte, bit in single_flips(k, m, nst):
        what = (kind, pos, t, byte, bit)
        if kind == "check":
            c2 = list(checks)
            c2[pos] = flipped(checks[pos], t, byte, bit)
            want = expected_flags(pred, check_mask, c2, nst)
            rule = np.zeros(nst, np.uint32)
            rule[t] = 1 << cb[pos]                    # exactly that brick's bit
            assert np.array_equal(want, rule), what
            verify(ins, c2, want, what)
        else:
            i2 = list(ins)
            i2[pos] = flipped(ins[pos], t, byte, bit)
            p2 = [p.copy() for p in pred]
            for i, chunk in enumerate(predict(O, k, n, mask, i2, [t])[t]):
                p2[i][t * CHUNK:(t + 1) * CHUNK] = chunk
            want = expected_flags(p2, check_mask, checks, nst)
            rule = np.zeros(nst, np.uint32)
            rule[t] = check_mask                      # every check brick's bit
            assert np.array_equal(want, rule), what
            verify(i2, checks, want, what)

    # two corrupted check bricks in the same stripe
    if m >= 2:
        t = nst // 2
        c2 = list(checks)
        c2[0] = flipped(checks[0], t, 200, 3)
        c2[m - 1] = flipped(checks[m - 1], t, 450, 6)
        want = expected_flags(pred, check_mask, c2, nst)
        assert want[t] == (1 << cb[0]) | (1 << cb[m - 1]) and np.count_nonzero(want) == 1
        verify(ins, c2, want, "two check bricks")
