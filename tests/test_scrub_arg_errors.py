"""The argument errors of the scrub family whose precedence the shared host
steps of ec_method.c decide: a misaligned loc / bad, an
avail_mask one brick short of what the call wants, a bit beyond the volume, a
target_mask that overlaps avail_mask and a NULL out[j].  Every call, host and
device entry, once with nstripes = 0 and once with nstripes = 1: the argument
checks come before the zero-stripes return and before anything looks at where
a buffer lives, so the answer is the same for both.  No GPU is needed (host
buffers at a device entry are -EINVAL with or without one).

EXPECTED was recorded from the library as it was before the shared steps were
written once (commit 575e747), not reasoned out: (return code with nstripes =
0, with nstripes = 1) per call and case.
"""
import ctypes
import errno

import numpy as np
import pytest

CHUNK = 512
K, N = 2, 7
AVAIL, TARGET = 0x3F, 0x40          # k + 4 bricks at hand, one to heal
E = -errno.EINVAL

# call -> (bricks avail_mask must name beside k, takes target_mask and out[])
CALLS = {
    "verify": (0, False), "locate": (2, False), "locate2": (4, False),
    "repair": (1, False), "repair2": (2, False),
    "decode_checked": (2, False), "decode_checked2": (4, False), "heal_checked": (2, True),
    "decode_verified": (1, False), "heal_verified": (1, True),
}
CASES = ("misaligned loc", "avail one short", "bit beyond the volume", "target overlaps avail",
         "out[j] NULL")

EXPECTED = {(call, case): (E, E) for call in CALLS for case in CASES
            if CALLS[call][1] or case not in ("target overlaps avail", "out[j] NULL")}


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def call(ec, L, name, device, nst, case):
    """One call that is valid but for `case`; returns (rc, buffers to keep)."""
    spare, heal = CALLS[name]
    frags = [np.zeros(CHUNK, np.uint8) for _ in range(N)]
    words = np.zeros(4, np.uint32)
    out = np.zeros(K * CHUNK, np.uint8)
    outs = [np.zeros(CHUNK, np.uint8)]
    avail, tmask = AVAIL, TARGET
    loc = words.ctypes.data + (2 if case == "misaligned loc" else 0)
    if case == "avail one short":
        avail = (1 << (K + spare - 1)) - 1
    elif case == "bit beyond the volume":
        avail |= 1 << N
    elif case == "target overlaps avail":
        tmask |= 1
    optr = ec._ptr_array([None] if case == "out[j] NULL" else outs)
    fn = getattr(ec.lib, "ec_method_" + name + ("_device" if device else ""))
    args = [ctypes.byref(L._list)] + ([0, None] if device else []) + [nst]
    cnt = [ctypes.c_uint64(77), ctypes.c_uint64(78)]
    if name == "verify":
        # mask = the k lowest bricks of avail, check_mask = the others
        short = case == "avail one short"
        mask = 0x1 if short else 0x3
        args += [mask, ec._ptr_array(frags[:K]), avail & ~0x3 if not short else 0x3C,
                 ec._ptr_array(frags[K:6]), loc]
        ncnt = 1
    elif name in ("locate", "locate2"):
        args += [avail, ec._ptr_array(frags), loc]
        ncnt = 1
    elif name in ("repair", "repair2"):
        args += [avail, ec._ptr_array(frags), loc]
        ncnt = 2
    elif name in ("decode_checked", "decode_checked2"):
        args += [avail, ec._ptr_array(frags), out.ctypes.data, loc]
        ncnt = 2
    elif name == "heal_checked":
        args += [avail, ec._ptr_array(frags), tmask, optr, loc]
        ncnt = 2
    elif name == "decode_verified":
        args += [avail, ec._ptr_array(frags), out.ctypes.data, loc]
        ncnt = 1
    else:
        args += [avail, ec._ptr_array(frags), tmask, optr, loc]
        ncnt = 1
    if not device:
        args += [ctypes.byref(c) for c in cnt[:ncnt]]
    rc = fn(*args)
    assert (cnt[0].value, cnt[1].value) == (77, 78), "a rejected call wrote its counters"
    assert not words.any() and not out.any() and not outs[0].any(), "a rejected call wrote"
    return rc


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,case", sorted(EXPECTED), ids=lambda v: v.replace(" ", "_"))
def test_argument_error_comes_first(ec, name, case, device):
    with ec.ECMatrixList(K, N, gen="none") as L:
        got = (call(ec, L, name, device, 0, case), call(ec, L, name, device, 1, case))
    assert got == EXPECTED[(name, case)], (name, case, device, got)
