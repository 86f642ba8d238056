"""The host-buffer family on the CPU engine (tests/_host_sweep.py): every call
of the table that tests/test_gpu_host_sweep.py sends through the GPU pipeline,
here with gen = none / avx and pageable buffers, through the same entry points
and the same runner (tests/_host_sweep_run.py), guards and input flanks
included.  No GPU is needed: this proves the table, its expected values (the
oracle's) and the runner on a machine without a device, and the restated
predicates branch(), encoder() and the batch size B against values worked out
by hand below.  The table's coverage clauses H1...H12 are asserted when
_host_sweep is imported.

The calls beside the GPU's size thresholds (series "thr", "d", "dmixed": up
to 64 MiB) mean nothing to the CPU engine and run with avx only.
"""
import numpy as np
import pytest

import _host_sweep as H
import _host_sweep_run as R

GENS = ["none", "avx"]
BIG = ("thr", "d", "dmixed")


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def pageable(cs):
    """Every distinct (shape, count) of the calls, all buffers pageable."""
    seen, out = set(), []
    for c in cs:
        key = (c.sh if c.sh[0] != "mixed" else id(c.sh[1]), c.nst, c.series)
        if key not in seen:
            seen.add(key)
            out.append(H.call(c.g, c.sh, c.nst, "G" * len(c.place), c.series))
    return out


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", H.GEOMS, ids=H.geom_id)
def test_host_sweep_cpu(ec, geom, gen):
    todo = [c for c in pageable(H.cases(geom)) if gen == "avx" or c.series not in BIG]
    arenas = R.Arenas(ec, "G")
    errs = R.run_cases(ec, geom, H.built(geom), todo, arenas, None, gen)
    assert not errs, "%d of %d calls: %s" % (len(errs), len(todo), errs[:5])


@pytest.mark.parametrize("geom", H.BATCH_GEOMS, ids=H.geom_id)
def test_host_sweep_batch_cases_cpu(ec, geom):
    todo = pageable(H.batch_cases(geom))
    errs = R.run_cases(ec, geom, H.built(geom, "batch"), todo, R.Arenas(ec, "G"), None, "avx")
    assert not errs, "%d of %d calls: %s" % (len(errs), len(todo), errs[:5])


def test_runner_sees_a_wrong_byte_and_a_stray_store(ec):
    """The runner reports a payload byte, a guard byte and an input byte."""
    g = (4, 6)
    c = [c for c in H.cases(g) if c.sh[0] == "dec" and c.nst == 9 and c.place == "GGGGG"][0]
    B = H.built(g)

    class Bad:
        def __init__(self, L, at):
            self.L, self.at = L, at

        def decode_batch(self, nst, mask, rows, inp, out):
            self.L.decode_batch(nst, mask, rows, inp, out)
            if self.at == "payload":
                out[700] ^= 1
            elif self.at == "guard":
                np.frombuffer((np.ctypeslib.ctypes.c_uint8 * 1).from_address(
                    out.ctypes.data + out.size + 4000), np.uint8)[0] = 0
            else:
                inp[1][3] ^= 1

    with ec.ECMatrixList(4, 6, gen="avx") as L:
        arenas = R.Arenas(ec, "G")
        assert R.run_call(L, B, c, arenas) == []
        for at, word in (("payload", "payload"), ("guard", "back guard"), ("input", "input")):
            errs = R.run_call(Bad(L, at), B, c, arenas)
            assert len(errs) == 1 and word in errs[0] and "4+2 dec" in errs[0], errs


# --- the restated predicates, against values worked out by hand --------------

def test_branch_by_hand():
    b = H.branch
    # 4+2: decode 2k + rows = 12, heal of 2 = 10: the k <= 4 persistent kernel
    assert b(4, 4, 13) == "A" and b(4, 2, 13) == "A" and b(4, 4, 13, zcdb=False) == "E"
    # 8+4: decode 16 + 8 = 24 <= 32; 8+12 encode: 16 + 20 = 36 > 32, 8 + 20 = 28 <= 32
    assert b(8, 8, 13) == "B" and b(8, 20, 13) == "E" and b(8, 25, 13) == "F"
    # 4+22 encode: 8 + 26 = 34 > 32, 4 + 26 = 30 <= 32, (4 + 26) * 4 KiB = 120 KiB
    assert b(4, 26, 13) == "E" and H.lds_e(4, 26) == 120 << 10
    assert b(4, 24, 13) == "A" and b(4, 25, 13) == "E" and b(4, 29, 13) == "F"
    # 16+4: heal of 4: 32 + 4 = 36 <= 39 (C); of 7: 39 (C); of 8: 40 (E below
    # 2048 stripes, D from 2048); decode 32 + 16 = 48: E / D
    assert [b(16, r, 13) for r in (1, 4, 7, 8, 16)] == ["C", "C", "C", "E", "E"]
    assert [b(16, r, 2048) for r in (7, 8, 16, 20, 31, 32)] == ["C", "D", "D", "D", "D", "D"]
    assert b(16, 16, 2047) == "E" and b(16, 20, 2047) == "F" and b(16, 31, 41) == "F"
    assert b(16, 16, 2048, zcdb=False) == "E" and b(16, 20, 4000, zcdb=False) == "F"
    # 9 + 12 / 9 + 13 encodes: 18 + 21 = 39 / 18 + 22 = 40
    assert b(9, 21, 13) == "C" and b(9, 22, 13) == "E" and b(9, 22, 2048) == "D"
    assert b(12, 31, 13) == "F" and b(12, 31, 2048) == "D"
    # groups below 8 stripes are sorted; 7+...: 2 * (1 + 7) = 16 words, 32 masks fit
    assert b(4, 4, 99, group=4) == "F" and b(4, 4, 99, group=8) == "A"
    assert b(7, 7, 99, group=8, npat=32) == "B" and b(7, 7, 99, group=8, npat=33) == "F"
    assert b(15, 15, 99, group=8, npat=8) == "E" and b(15, 15, 99, group=8, npat=9) == "F"
    assert b(3, 3, 99, group=8, npat=128) == "A" and b(3, 3, 99, group=8, npat=129) == "F"


def test_encoder_by_hand():
    e = H.encoder
    # 4 * 32 * 256 = 32768 units of 16 / W stripes: 2+1 (W = 4) above 8192,
    # 4+2 (W = 2) above 4096, 8+4 and 16+4 (W = 1) above 2048
    assert [e(2, 3, c) for c in (8192, 8193)] == ["vander", "vander_zc"]
    assert [e(4, 6, c) for c in (4096, 4097)] == ["vander", "vander_zc"]
    assert [e(8, 12, c) for c in (2048, 2049)] == ["vander", "vander_zc"]
    assert [e(16, 20, c) for c in (2047, 2048, 8191, 8192)] == \
        ["vander", "combine", "combine", "vander_zc"]
    assert [e(16, 20, c, zcenc16=False) for c in (2048, 2049)] == ["vander", "vander_zc"]
    assert e(5, 7, 13) == "combine" and e(16, 31, 9000) == "combine"


def test_batch_by_hand():
    # 4+2 encode: 2 KiB of input per stripe; 32 MiB = 16384 stripes staged,
    # 256 MiB = 131072 in place
    assert H.cut(40000, H.batch(True, 40000, 2048, False)) == [16384, 16384, 7232]
    assert H.batch(True, 40000, 2048, True) == 40000
    assert H.cut(153600, H.batch(True, 153600, 2048, True)) == [131072, 22528]
    # a single staged batch of 4 MiB is cut in 4 of 1 MiB, of 3 MiB + 1 stripe in 3
    assert H.cut(2048, H.batch(True, 2048, 2048, False)) == [512] * 4
    assert H.cut(1537, H.batch(True, 1537, 2048, False)) == [513, 513, 511]
    assert H.cut(1023, H.batch(True, 1023, 2048, False)) == [1023]
    # 8+4 decode: 8 fragments of 512 bytes per stripe: 8192 stripes staged
    assert H.cut(20000, H.batch(False, 20000, 4096, False)) == [8192, 8192, 3616]
    # 16+4 decode: 4096 stripes staged; a mixed decode reads all 20 fragments:
    # 32 MiB / 10240 = 3276, rounded down to groups of 64: 3264
    assert H.cut(9000, H.batch(False, 9000, 8192, False)) == [4096, 4096, 808]
    assert H.batch(False, 9000, 10240, False, group=64) == 3264
    # 1 MiB batches: 16+4 encodes in launches of 128 stripes, 4+2 of 512
    assert H.batch(True, 9000, 8192, False, 1) == 128 and H.batch(True, 9000, 2048, False, 1) == 512
    assert H.batch(True, 9000, 8192, True, 1) == 1024


def test_launches_and_kernels_of_calls():
    c = H.call((16, 20), ("enc",), 3000, "G" * 21, "x")
    assert H.launches_of(c) == [750] * 4 and H.kernels_of(c) == {"vander"}
    c = H.call((16, 20), ("enc",), 3000, "P" * 21, "x")
    assert H.launches_of(c) == [3000] and H.kernels_of(c) == {"D"}
    assert H.kernels_of(c, zcenc16=False) == {"vander_zc"}
    c = H.call((4, 6), ("rows", 0x3F), 5000, "P" * 7, "x")
    assert H.kernels_of(c) == {"vander_zc"}
    c = H.call((4, 6), ("rows", 0x30), 5000, "P" * 3, "x")
    assert H.kernels_of(c) == {"A"} and H.kernels_of(c, zcdb=False) == {"E"}
