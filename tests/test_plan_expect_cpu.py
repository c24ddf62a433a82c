"""The expectation helper of the plan lifecycle tests (tests/plan_cases.py),
checked on the CPU: for every small shape and each of its bad sets, the
oracle's chunk CRCs of the corrupted bytes differ from the expected CRC arrays
as uploaded in exactly the intended chunks, and first_bad, the count and the
bitmap bytes follow from that set; the sets have the properties the verify
sequence relies on; the size rule names the launch class each shape is built
for at several CU counts."""
import numpy as np
import pytest

import plan_cases as pc
from oracle import splitmix64_np

CUS = (256, 304, 128, 64)


@pytest.mark.parametrize("which", ["clean", "a", "b"])
@pytest.mark.parametrize("shape", pc.SMALL_SHAPES)
def test_expectation_from_the_sets_alone(oracle, shape, which):
    case = pc.build(shape, 256, seed=3)
    case.make_host(oracle)
    bad = {"clean": {}, "a": case.a, "b": case.b}[which]
    data, crcs = case.data_image(bad), case.crc_image(bad)
    differ, fb = set(), [pc.NONE] * len(case.segs)
    for i, s in enumerate(case.segs):
        if not s.nchunks:
            continue
        got = oracle.chunk_crcs(data[s.data_at:s.data_at + s.len], s.cs)
        want = crcs[s.crc_at:s.crc_at + 4 * s.nchunks].view(">u4").astype(np.uint32)
        for c in np.flatnonzero(got != want):
            differ.add((i, int(c)))
            fb[i] = min(fb[i], int(c))
    assert differ == set(bad)
    assert fb == case.first_bad(bad) and case.count(bad) == len(differ)
    # the bitmap image: guards outside, exactly the bad chunks' bits inside
    img = case.bitmap_image(bad)
    inside = np.zeros(case.bm_size, dtype=bool)
    for i, s in enumerate(case.segs):
        if s.nchunks:
            inside[s.bm_at:s.bm_at + s.bm_bytes] = True
            bits = np.unpackbits(img[s.bm_at:s.bm_at + s.bm_bytes], bitorder="little")
            assert sorted(int(c) for c in np.flatnonzero(bits)) == sorted(c for t, c in bad if t == i)
    assert (img[~inside] == pc.GUARD).all()
    # one flip per bad chunk and nothing else: the images differ from the clean ones in len(bad) bytes
    assert int((data != case.data_image()).sum()) == sum(k == "data" for k in bad.values())
    assert int((crcs != case.crc_image()).sum()) == sum(k == "crc" for k in bad.values())


@pytest.mark.parametrize("shape", pc.SMALL_SHAPES)
def test_layout_keeps_guards_between_neighbours(oracle, shape):
    case = pc.build(shape, 256)
    case.make_host(oracle)
    live = [s for s in case.segs if s.nchunks]
    for x, y in zip(live, live[1:]):
        assert y.bm_at - (x.bm_at + x.bm_bytes) >= 1
        assert y.crc_at - (x.crc_at + 4 * x.nchunks) >= 4 * pc.CRC_GAP_WORDS and y.crc_at % 4 == 0
        assert y.data_at - (x.data_at + x.len) >= pc.DATA_GAP
    for s in live:
        assert s.data_at % 16 == s.residue
    assert live[0].bm_at >= 1 and case.bm_size > live[-1].bm_at + live[-1].bm_bytes
    for img, at, n in ((case.data_image(), [s.data_at for s in live], [s.len for s in live]),
                       (case.crc_image(), [s.crc_at for s in live], [4 * s.nchunks for s in live])):
        mask = np.ones(img.size, dtype=bool)
        for a, k in zip(at, n):
            mask[a:a + k] = False
        assert (img[mask] == pc.GUARD).all()


@pytest.mark.parametrize("num_cu", CUS)
@pytest.mark.parametrize("shape", pc.SHAPES)
def test_sets_and_launch_class(shape, num_cu):
    case = pc.build(shape, num_cu)
    pc.check_sets(case, case.a, case.b, pool=shape >= 4)
    for compute in (False, True):
        k = pc.check_class(case, num_cu, compute)
        assert k["nchunks"] == sum(s.nchunks for s in case.segs)
    if shape >= 4:   # 640 MiB at 256 CUs
        assert k["main_bytes"] >= pc.pool_rounds(num_cu) * 4096
        assert k["main_bytes"] < pc.pool_rounds(num_cu) * 4096 + (16 << 20)


def test_formula_bytes_match_the_fill():
    """chunk_bytes() regenerates what the device fill writes: segment s holds
    splitmix64(seed, g0_s + k), 64 words per 512-B chunk."""
    case = pc.build(5, 8, seed=9)
    picks = [(0, 0), (1, 87), (len(case.segs) - 1, case.segs[-1].nchunks - 1)]
    got = case.chunk_bytes(picks)
    for j, (s, c) in enumerate(picks):
        want = splitmix64_np(64, seed=9, g0=case.segs[s].g0 + 64 * c).view(np.uint8)
        assert np.array_equal(got[512 * j:512 * (j + 1)], want)
    sm = case.samples()
    assert len(sm) >= 200 and {(i, 0) for i in range(len(case.segs))} <= set(sm)
    assert {(i, s.nchunks - 1) for i, s in enumerate(case.segs)} <= set(sm)
