"""The encode family on device buffers (tests/_encode_sweep.py): encode_device
for 2+1, 4+2, 8+4 and 16+4 and writev_encode_device for those four, 5+2 and
10+3, with

  - every stripe count from 1 to 9 (every ragged tile of the 4-stripe tile
    encoders), the register encoders' block size and its neighbours, and 259;
  - the input at every address modulo 16 at 9, 6 and 7 stripes, so
    stage_tile_shift at every byte shift with a ragged tile of 1, 2 and 3
    stripes, and every fragment at an address of its own;
  - writes at every head and end of the table with the tail edge stripe in
    every tile slot, ranges inside one 16-byte piece of ec_rmw_gather, an end
    on a stripe boundary with old_tail given, every presence of the old
    stripes, and the interior at every address modulo 16.

By default 4+2 and 8+4 run ec_encode_tile_t and 16+4 ec_encode_tile_rb
(LDS-DMA staging, SM = 0 / 1, or shift staging, SM = 3, where the input is
not dword-aligned) and 2+1 ec_encode_vander / ec_encode_vander_rmw<..., 1>;
5+2 and 10+3 gather the whole padded buffer and run the generic combine.
test_encode_sweep_register_encoders runs the four compile-time geometries in
a child process with EC_MI355X_ENC=0 (read when the library first encodes):
ec_encode_vander<K, N, W> and ec_encode_vander_rmw<K, N, W, 1> for 4+2, 8+4
and 16+4 too.  test_encode_sweep_nontemporal runs their plain encodes in a
child with EC_MI355X_LDSNT=1: the non-temporal tile encoders wherever the
input is 16-byte aligned; nothing is asserted about which kernel ran.

The expected values come from the oracle, never from the library.  Every call
of a geometry is queued on one side stream with one sync, and every device
tensor of a call is held until after that sync.  The outputs of a call are
slices of one allocation pre-filled with 0xA5 with 2 KiB of guard on both
sides of each; the inputs sit between 64-byte flanks and are compared with
their uploaded bytes after the sync.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _encode_sweep as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


class Call:
    """One case on the device: its uploaded inputs, its output allocation and
    the views the library gets."""

    def __init__(self, x, what):
        import torch
        self.x, self.what = x, what
        self.din = torch.from_numpy(np.array(x.ibuf)).to(DEV)   # (ibuf is read-only)
        self.dout = torch.full((x.lay.total,), W.FILL, dtype=torch.uint8, device=DEV)
        self.outs = [self.dout[start:start + size] for _, start, size, _ in x.lay.seg]
        assert self.din.data_ptr() % 16 == 0 and self.dout.data_ptr() % 16 == 0

    def view(self, start, size):
        return None if start is None else self.din[start:start + size]

    def errors(self):
        errs = W.check_outputs(self.dout.cpu().numpy(), self.x.lay, self.x.want)
        if not np.array_equal(self.din.cpu().numpy(), self.x.ibuf):
            errs.append(("an input or its flank was written",))
        return errs


def plain_calls(S):
    calls = []
    for x in S.plain:
        c = Call(x, W.plain_id(x.c))
        c.inp = c.view(x.iseg[0], S.S * x.c.nst)
        assert c.inp.data_ptr() % 16 == x.c.off
        assert [o.data_ptr() % 16 for o in c.outs] == list(x.c.outs)
        calls.append(c)
    return calls


def write_calls(S, cases=None):
    calls = []
    for x in S.writes if cases is None else cases:
        c = Call(x, W.write_id(x.c))
        c.user = c.view(x.user, x.c.size)
        c.oh, c.ot = c.view(x.oh, S.S), c.view(x.ot, S.S)
        assert (c.user.data_ptr() - x.c.head) % 16 == W.interior_shift(x.c)
        calls.append(c)
    return calls


def failures(calls):
    return [(c.what, e) for c in calls for e in c.errors()]


def sweep(ec, geom, plain=True, writes=True):
    """Every device call of one geometry on one side stream, one sync, then
    the comparisons."""
    import torch
    S = W.built(geom)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    with ec.ECMatrixList(S.k, S.n) as L:
        enc = plain_calls(S) if plain and geom in W.ENC_GEOMS else []
        wr = write_calls(S) if writes else []
        assert enc or wr
        torch.cuda.synchronize()
        for c in enc:
            L.encode_device(0, s, c.x.c.nst, c.inp, c.outs)
        for c in wr:
            L.writev_encode_device(0, s, c.x.c.head, c.x.c.size, c.user, c.oh, c.ot, c.outs)
        ec.sync_device(0, s)
        bad = failures(enc + wr)            # enc and wr still hold every tensor
    assert not bad, (W.geom_id(geom), len(bad), bad[:6])


@pytest.mark.parametrize("geom", W.WRITE_GEOMS, ids=W.geom_id)
def test_encode_sweep_device(ec, geom):
    sweep(ec, geom)


@pytest.mark.parametrize("geom", W.WRITE_GEOMS, ids=W.geom_id)
def test_writev_sweep_host_entry_device_pointers(ec, geom):
    """ec_method_writev_encode with device pointers (it finds the device and
    syncs itself): one multi-stripe and one single-stripe case, both with the
    user range strictly inside its edge stripes and both old stripes given."""
    import torch
    S = W.built(geom)
    multi = next(x for x in S.writes if x.c.nst > 4 and x.c.oh and x.c.ot and
                 x.c.head and x.c.b2 % S.S and W.interior_shift(x.c) % 4)
    one = next(x for x in S.writes if x.c.nst == 1 and x.c.oh and x.c.ot and
               x.c.head and x.c.b2 < S.S)
    calls = write_calls(S, [multi, one])
    torch.cuda.synchronize()
    with ec.ECMatrixList(S.k, S.n) as L:
        for c in calls:
            L.writev_encode(c.x.c.head, c.user, c.oh, c.ot, c.outs)
    bad = failures(calls)
    assert not bad, (W.geom_id(geom), bad[:6])


# --- the other instantiations: the same sweep in a child process -------------

CHILD = r"""
import sys
sys.path[:0] = ["tests", "oracle"]
import glusterfs_amd.ec_method as ec
import _encode_sweep as W
import test_gpu_encode_sweep as T
bad = []
for g in W.ENC_GEOMS:
    try:
        T.sweep(ec, g, writes=sys.argv[1] == "writes")
    except AssertionError as e:             # wrong bytes: say so for every geometry
        bad.append(str(e)[:700])
if bad:
    sys.exit("\n".join(bad))
print("ok")
"""


def child(knob, value, writes):
    env = dict(os.environ, EC_MI355X_QUIET="1")
    env[knob] = value
    r = subprocess.run([sys.executable, "-c", CHILD, "writes" if writes else "plain"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


def test_encode_sweep_register_encoders():
    """EC_MI355X_ENC=0: ec_encode_vander<K, N, W> for the plain encodes and
    ec_encode_vander_rmw<K, N, W, 1> for the writes of all four geometries."""
    child("EC_MI355X_ENC", "0", True)


def test_encode_sweep_nontemporal():
    """EC_MI355X_LDSNT=1: the plain encodes again; the aligned ones (every
    count from 1 to 9 among them) stage with non-temporal loads, the others
    keep the default policy."""
    child("EC_MI355X_LDSNT", "1", False)
