"""ec_method_decode_verified_device and ec_method_heal_verified_device over the
whole table of tests/_verified_sweep.py: ec_decode_verified_n and
ec_heal_verified_n with the run-time k at every value of each K bucket (1...4,
5...8, 9...16), every count of check rows from 1 to 15 (and 18), wave-item
counts on both sides of the block's wave count, coefficient tables up to the
124 words of a read of 31 bricks, bases that reach brick 24 and above, check
bricks that are not contiguous and targets below, between and above the basis
bricks.  One geometry per bucket runs again with every fragment and output 1
byte into its allocation and bad[] at each dword offset modulo 16, and every
geometry runs again in a child process with non-temporal staging
(EC_MI355X_LDSNT=1).  The 4-wave instantiations of 5 <= k <= 8 (above 2^17
stripes) stay with tests/test_gpu_verified.py.

The expected values come from the oracle and include/ec_method.h, never from
the library; on every call bad[] also equals ec_method_verify_device with B
and C and the output ec_method_decode_device / ec_method_heal_device with
mask B.  bad[] is pre-filled with 0xFFFFFFFF between guard words, outputs with
0xA5 and a guard chunk, and no fragment may change, nor the buffer of any
brick outside avail_mask.
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _verified_sweep as W

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


def new_bad(nst, word=0):
    """bad[0 .. nst) `word` dwords into a 16-byte aligned allocation, with
    guard words on both sides: (the whole tensor, the view to pass)."""
    import torch
    t = torch.full((word + nst + W.GUARD,), -1, dtype=torch.int32, device=DEV)
    assert t.data_ptr() % 16 == 0
    return t, t[word:]


def read_bad(bad, nst, word=0):
    got = bad[0].cpu().numpy().view(np.uint32)
    assert (got[:word] == W.SENTINEL).all() and (got[word + nst:] == W.SENTINEL).all(), \
        "guard words written"
    return got[word:word + nst].copy()


def new_out(chunks, offset=0):
    """`chunks` chunks and a guard chunk of 0xA5, `offset` bytes into the
    allocation."""
    import torch
    t = torch.full((W.CHUNK * (chunks + 1) + offset,), W.FILL, dtype=torch.uint8, device=DEV)
    return t[offset:]


def read_out(out, chunks):
    got = out.cpu().numpy()
    assert (got[W.CHUNK * chunks:] == W.FILL).all(), "guard chunk written"
    return got[:W.CHUNK * chunks].copy()


def sweep(ec, geom, off):
    """The read and every heal of one geometry, each beside the plain calls
    that define it, queued on one side stream with one sync.  Every fragment
    and output starts `off` bytes into its allocation; with off != 0 the
    bad[] of call i starts i % 4 dwords into its own."""
    import torch
    S = W.built(geom)
    k, n, nst, am = S.k, S.n, S.nst, S.avail_mask
    filler = np.full(W.CHUNK * nst, 0x3C, np.uint8)
    # bricks outside avail_mask, the targets among them, get a buffer of their
    # own in frags[]: nothing may read or write it
    dfr = [dev(filler if f is None else f, off) for f in S.frags]
    ins, chk = [dfr[b] for b in S.basis], [dfr[b] for b in S.checks]
    st = torch.cuda.Stream()
    s = st.cuda_stream
    held = []                       # every tensor of every call, until after the sync
    for i, targets in enumerate((None,) + S.heals):
        per = k if targets is None else 1
        word = i % 4 if off else 0
        held.append(SimpleNamespace(
            targets=targets, per=per, word=word, bad=new_bad(nst, word),
            out=[new_out(per * nst, off) for _ in (targets or (0,))],
            ref=[new_out(per * nst) for _ in (targets or (0,))]))
    bad_ref = new_bad(nst)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        for c in held:
            if c.targets is None:
                L.decode_verified_device(0, s, nst, am, dfr, c.out[0], c.bad[1])
                L.decode_device(0, s, nst, S.bmask, ins, c.ref[0])
            else:
                tm = W.mask_of(c.targets)
                L.heal_verified_device(0, s, nst, am, dfr, tm, c.out, c.bad[1])
                L.heal_device(0, s, nst, S.bmask, ins, tm, c.ref)
        L.verify_device(0, s, nst, S.bmask, ins, S.cmask, chk, bad_ref[1])
        ec.sync_device(0, s)
    ref = read_bad(bad_ref, nst)
    for c in held:
        what = (W.geom_id(geom), c.targets, off)
        bad = read_bad(c.bad, nst, c.word)
        outs = [read_out(o, c.per * nst) for o in c.out]
        W.compare(S, c.targets, bad, outs, None, what)
        assert np.array_equal(bad, ref), (what, "bad differs from ec_method_verify_device")
        for o, h in zip(outs, c.ref):
            assert np.array_equal(o, read_out(h, c.per * nst)), \
                (what, "differs from the plain call with mask B")
    for b, (d, f) in enumerate(zip(dfr, S.frags)):
        assert np.array_equal(d.cpu().numpy(), filler if f is None else f), \
            "the buffer of brick %d was written" % b


@pytest.mark.parametrize("geom", W.SWEEP, ids=W.geom_id)
def test_verified_sweep_device(ec, geom):
    sweep(ec, geom, 0)


@pytest.mark.parametrize("geom", W.offset_geoms(), ids=W.geom_id)
def test_verified_sweep_device_buffers_at_odd_addresses(ec, geom):
    """k = 3, 7 and 11: every fragment and every output 1 byte into its
    allocation; the four calls' bad[] at the four dword offsets modulo 16."""
    assert len(geom[3]) == 3
    sweep(ec, geom, 1)


# --- the non-temporal copies: the same sweep with EC_MI355X_LDSNT=1 ----------

CHILD = r"""
import sys
sys.path[:0] = ["tests", "oracle"]
import glusterfs_amd.ec_method as ec
import _verified_sweep as W
import test_gpu_verified_sweep as T
failed = 0
for g in W.bucket_geoms(int(sys.argv[1])):
    try:
        T.sweep(ec, g, 0)
        print("geom %s ok" % W.geom_id(g), flush=True)
    except AssertionError as e:
        failed = 1
        print("geom %s FAILED %s" % (W.geom_id(g), str(e)[:300].replace("\n", " ")), flush=True)
sys.exit(failed)
"""


@pytest.mark.parametrize("K", [4, 8, 16])
def test_verified_sweep_nontemporal(K):
    """One child per K bucket (EC_MI355X_LDSNT is read when the library
    loads): every geometry of the bucket at 16-byte aligned addresses, so
    both kernels stage with non-temporal loads; one result line each."""
    env = dict(os.environ, EC_MI355X_QUIET="1", EC_MI355X_LDSNT="1")
    r = subprocess.run([sys.executable, "-c", CHILD, str(K)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=170)
    lines = r.stdout.splitlines()
    for g in W.bucket_geoms(K):
        assert "geom %s ok" % W.geom_id(g) in lines, \
            (W.geom_id(g), [x for x in lines if "FAILED" in x][:4], r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
