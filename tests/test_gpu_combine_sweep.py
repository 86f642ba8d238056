"""The combine family on device buffers over every k from 1 to 16
(tests/_combine_sweep.py): decode_device, heal_device, decode_mixed_device,
encode_device and encode_rows_device, all of which run ec_combine_n (k <= 8)
or ec_combine (k > 8) through ecdk_combine / combine_any<true>, with

  - the run-time k at every value of each K bucket (1...4, 5...8, 9...16):
    the staging loop's p >= k break, the partial last coefficient word, the
    output slices behind k inputs;
  - heals of 1, 2, a drawn number and all n - k bricks, so fewer rows than
    waves, a second and a third pass over the waves, rows > k, and encodes of
    up to 31 rows (16+15: one pattern of exactly 128 words);
  - every launch shape per bucket: single pattern, tile-mixed and sorted
    slots, each with the masks in the kernel arguments and in the device
    table, 8 masks of 15+16 (exactly 512 words) beside 9;
  - every buffer, the group map included, 1 byte into its allocation for one
    geometry per bucket.

test_combine_sweep_nontemporal runs the same sweep in a child process with
EC_MI355X_LDSNT=1 (read when the library loads): the kLdsDmaNT copy of every
kernel above; the 1-byte-off variant falls back to the default policy there.
test_combine_at_scale launches the 4-wave K = 8 instantiations, which take
more than 2^17 stripes.

The expected values come from the oracle, never from the library.  Outputs
are pre-filled with 0xA5 and followed by a guard chunk, and the inputs are
compared with their uploaded bytes after the calls.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _combine_sweep as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def new_out(chunks, offset=0):
    """`chunks` chunks and a guard chunk of 0xA5, `offset` bytes into the
    allocation."""
    import torch
    t = torch.full((W.CHUNK * (chunks + 1) + offset,), W.FILL, dtype=torch.uint8, device=DEV)
    return t[offset:]


def read_out(out, chunks):
    got = out.cpu().numpy()
    assert (got[W.CHUNK * chunks:] == W.FILL).all(), "guard chunk written"
    return got[:W.CHUNK * chunks]


def same(got, want, width, what):
    d = np.flatnonzero((got.reshape(-1, width) != want.reshape(-1, width)).any(axis=1))
    assert d.size == 0, (what, "stripes", d[:8].tolist())


def sweep(ec, geom, off):
    """Every device call of one geometry on one side stream, one sync, then
    the comparisons; every buffer starts `off` bytes into its allocation."""
    import torch
    S = W.built(geom)
    k, n, C, nst = S.k, S.n, S.C, W.NST
    kc = k * W.CHUNK
    st = torch.cuda.Stream()
    s = st.cuda_stream
    with ec.ECMatrixList(k, n) as L:
        fr = [dev(f, off) for f in S.frags]
        data = dev(S.data, off)
        mfr = [dev(f, off) for f in S.mfr]
        ids = [dev(x.ids, off) for x in C.mixed]
        dec = [new_out(k * nst, off) for _ in C.decode]
        heal = [[new_out(nst, off) for _ in W.bits(t)] for _, t in C.heal]
        enc = [new_out(nst, off) for _ in range(n)]
        rows = [[new_out(nst, off) if (rm >> b) & 1 else None for b in range(n)]
                for rm in C.row_masks]
        mixed = [new_out(k * x.nst, off) for x in C.mixed]
        torch.cuda.synchronize()
        for m, o in zip(C.decode, dec):
            L.decode_device(0, s, nst, m, [fr[b] for b in W.bits(m)], o)
        for (m, t), outs in zip(C.heal, heal):
            L.heal_device(0, s, nst, m, [fr[b] for b in W.bits(m)], t, outs)
        L.encode_device(0, s, nst, data, enc)
        for rm, outs in zip(C.row_masks, rows):
            L.encode_rows_device(0, s, nst, data, rm, outs)
        for x, gp, o in zip(C.mixed, ids, mixed):
            L.decode_mixed_device(0, s, x.nst, x.group, gp, x.masks, mfr, o)
        ec.sync_device(0, s)

        for m, o in zip(C.decode, dec):
            same(read_out(o, k * nst), S.dec[m], kc, ("decode", hex(m)))
        for (m, t), outs in zip(C.heal, heal):
            for b, o, want in zip(W.bits(t), outs, S.heal[m, t]):
                same(read_out(o, nst), want, W.CHUNK, ("heal", hex(m), hex(t), b))
        for b, o in enumerate(enc):
            same(read_out(o, nst), S.enc[b], W.CHUNK, ("encode", b))
        for rm, outs in zip(C.row_masks, rows):
            for b in W.bits(rm):
                same(read_out(outs[b], nst), S.enc[b], W.CHUNK, ("encode_rows", hex(rm), b))
        for x, o, want in zip(C.mixed, mixed, S.mixed):
            same(read_out(o, k * x.nst), want, kc,
                 ("mixed", W.shape(k, x), x.group, len(x.masks)))
        for what, got, want in (("fragment", fr, S.frags), ("data", [data], [S.data]),
                                ("mixed fragment", mfr, S.mfr),
                                ("group map", ids, [x.ids for x in C.mixed])):
            for i, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g.cpu().numpy(), w), "%s %d was written" % (what, i)


@pytest.mark.parametrize("geom", W.GEOMS, ids=W.geom_id)
def test_combine_sweep_device(ec, geom):
    sweep(ec, geom, 0)


@pytest.mark.parametrize("geom", W.OFFSET_GEOMS, ids=W.geom_id)
def test_combine_sweep_device_buffers_at_odd_addresses(ec, geom):
    sweep(ec, geom, 1)


# --- the non-temporal copies: the same sweep with EC_MI355X_LDSNT=1 ----------

CHILD = r"""
import sys
sys.path[:0] = ["tests", "oracle"]
import glusterfs_amd.ec_method as ec
import _combine_sweep as W
import test_gpu_combine_sweep as T
K = int(sys.argv[1])
for g in W.GEOMS:
    if W.bucket(g[0]) == K:
        T.sweep(ec, g, 0)
        if g in W.OFFSET_GEOMS:
            T.sweep(ec, g, 1)
print("ok")
"""


@pytest.mark.parametrize("K", [4, 8, 16])
def test_combine_sweep_nontemporal(K):
    """One child per K bucket: every geometry of it, and the one with every
    buffer 1 byte off (default policy again, through inputs_aligned)."""
    env = dict(os.environ, EC_MI355X_QUIET="1", EC_MI355X_LDSNT="1")
    r = subprocess.run([sys.executable, "-c", CHILD, str(K)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


# --- the 4-wave bucket: 5 <= k <= 8 above 2^17 stripes -----------------------

BIG = (5, 9, (1 << 17) + 5)


@pytest.fixture(scope="module")
def big(oracle):
    """5+4 fragments of 2^17 + 5 stripes, oracle-encoded once; the first seven
    are the fragments of the 5+2 volume (a brick's row of the encode matrix
    depends on k and the brick alone: checked on the first stripes)."""
    k, n, nst = BIG
    rng = np.random.default_rng(529)
    data = rng.integers(0, 256, W.CHUNK * k * nst, dtype=np.uint8)
    frags = oracle.encode(k, n, data, nthreads=8)
    for f, g in zip(oracle.encode(k, 7, data[:W.CHUNK * k * 8]), frags):
        assert np.array_equal(f, g[:W.CHUNK * 8])
    return data, frags                                      # dropped with the module


@pytest.mark.parametrize("off", [0, 1], ids=["aligned-nt", "offset-default"])
def test_combine_at_scale(ec, big, off):
    """5+2, the smallest k of the bucket, at 2^17 + 5 stripes (64 MiB per
    fragment; the size is the dispatch condition): above 2^17 stripes k in
    5...8 runs 4 waves per block.  Single-pattern decode, a heal of both
    missing bricks (fewer rows than waves), mixed decode with groups of 2
    (sorted) and of 4096 (tile-mixed), and both again with 45 masks of 5+4,
    more than the 42 that fit the kernel arguments (device table).  Aligned
    fragments: every call reads 320 MiB and stages with non-temporal loads;
    fragments 1 byte off: default-policy loads.  The fragments are the
    encoding of the data, so every decode gives the data: compared on the
    device."""
    import torch
    data, frags = big
    k, n9, nst = BIG
    kc = k * W.CHUNK
    rng = np.random.default_rng(530)
    dfr = [dev(f, off) for f in frags]
    exp = torch.from_numpy(data).to(DEV)
    out = new_out(k * nst, off)

    def check(what):
        ec.sync_device(0)
        assert torch.equal(out[:kc * nst], exp), what
        assert (out[kc * nst:] == W.FILL).all(), (what, "guard chunk written")
        out.fill_(W.FILL)
        torch.cuda.synchronize()

    torch.cuda.synchronize()
    with ec.ECMatrixList(k, 7) as L:
        m = 0b1011101                                       # bricks 1 and 5 are missing
        src = [dfr[b] for b in W.bits(m)]
        L.decode_device(0, None, nst, m, src, out)
        check("decode")
        h1, h5 = new_out(nst, off), new_out(nst, off)
        L.heal_device(0, None, nst, m, src, 0b0100010, [h1, h5])
        ec.sync_device(0)
        for b, h in ((1, h1), (5, h5)):
            assert torch.equal(h[:W.CHUNK * nst], dfr[b]), ("heal", b)
            assert (h[W.CHUNK * nst:] == W.FILL).all(), ("heal", b, "guard chunk written")
        del h1, h5
        masks = W.draw_masks(k, 7, 21, 1)
        assert len(masks) * W.pwords(k) <= W.ARG_WORDS
        for group in (2, 4096):
            ids = rng.integers(0, len(masks), -(-nst // group)).astype(np.uint8)
            L.decode_mixed_device(0, None, nst, group, dev(ids, off), masks, dfr[:7], out)
            check(("mixed, kernel arguments", group))
    with ec.ECMatrixList(k, n9) as L:
        masks = W.draw_masks(k, n9, 45, 1)
        assert len(masks) * W.pwords(k) > W.ARG_WORDS
        for group in (2, 4096):
            ids = rng.integers(0, len(masks), -(-nst // group)).astype(np.uint8)
            ids[:len(masks)] = np.arange(len(masks))[:len(ids)]    # the masks of the table
            L.decode_mixed_device(0, None, nst, group, dev(ids, off), masks, dfr, out)
            check(("mixed, device table", group))
    del exp, out
    for b, f in enumerate(frags):
        assert torch.equal(dfr[b], torch.from_numpy(f).to(DEV)), "fragment %d was written" % b
    del dfr
    torch.cuda.empty_cache()
