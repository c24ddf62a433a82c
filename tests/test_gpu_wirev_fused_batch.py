"""GPU: the wire streams of a batch of writes, each held in a list of device
buffers, made in one call, one launch and one pass
(include/hadoofus_wirev_fused_batch.h) -- frame_fused_gather_batch_kernel walks
the packets of all writes, finds every round's write and then its fragment in
that write's slice of one fragment table, copies the bytes, computes the chunk
CRCs from the registers it copies and writes every byte of every stream.

The expected stream of every write is built on the host from the CPU oracle
(gather_arena.expect of the write's concatenation).  Fragments and
destinations are carved from one device allocation between 0xA5 guards, at
chosen byte residues mod 16; after every call the whole allocation is
downloaded and compared with the image expected, so the fragments and the
guards are untouched and every destination equals its expected stream.  Where
a test claims a path of the kernel, it first asks the layout call whether its
shape takes it.  Unless a case says otherwise it runs on the product's grid
and, through the timing call, on 1, 3 and 7 workgroups.  Everything is
bit-exact."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from gather_arena import Arena, cut, expect, room
from packet_stream import payload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
N2 = 2 * 65536 + 700  # at 4321: packets of 287, 65536, 65536 and 413 bytes
GROUPS = (1, 3, 7)


@pytest.fixture(scope="module")
def wvb(engine):
    from hadoofus_amd import wirev_fused_batch
    wirev_fused_batch.load()
    return wirev_fused_batch


def spec(seed, lens, off=0, seq=0, finish=False, mis=(0,), dst_mis=0, data=None):
    """One write of a batch: `lens` bytes per fragment of payload(seed)."""
    d = payload(seed, 0, sum(lens)) if data is None else data
    return dict(d=d, lens=list(lens), off=off, seq=seq, finish=finish, mis=mis, dst_mis=dst_mis)


def wants(oracle, specs, proto=2, ctype=2):
    return [expect(oracle, s["d"], s["off"], s["seq"], proto, ctype, s["finish"]) for s in specs]


def arena_for(engine, specs, want, slack=0):
    return Arena(engine, room(sum(len(s["d"]) for s in specs) + sum(len(w[0]) for w in want) + slack,
                              sum(len(s["lens"]) for s in specs) + len(specs)))


def lay(arena, specs, want):
    """Every write's fragments (fragment i of a write at residue mis[i %
    len(mis)]), then every write's destination.  -> the batch's write dicts."""
    arena.begin()
    frags = [[(arena.put(p, s["mis"][i % len(s["mis"])]), len(p)) for i, p in enumerate(cut(s["d"], s["lens"]))]
             for s in specs]
    writes = [dict(frags=f, wire_ptr=arena.wire(len(w[0]), s["dst_mis"]), wire_cap=len(w[0]),
                   offset_in_block=s["off"], seqno=s["seq"], finish=s["finish"])
              for f, s, w in zip(frags, specs, want)]
    arena.commit()
    return writes


def run(wvb, arena, specs, want, proto=2, ctype=2, groups=GROUPS):
    """The call on the product's grid, then the timing call on each of
    `groups` workgroups; the whole arena compared after each."""
    streams = [w[0] for w in want]
    writes = lay(arena, specs, want)
    assert wvb.compose(writes, proto, ctype) == [(len(w[0]), w[1]) for w in want]
    arena.check(streams)
    for g in groups:
        arena.commit()  # guards over the streams again
        ms = wvb.fused_batch_time(writes, proto, ctype, wvb.time_groups(g), 1)
        assert (ms > 0) == any(w[1] for w in want)  # no packet, no launch
        arena.check(streams)
    return writes


def totals(wvb, specs, proto=2, ctype=2):
    return wvb.layout([dict(frags=[(None, n) for n in s["lens"]], offset_in_block=s["off"], finish=s["finish"])
                       for s in specs], proto, ctype)[1]


# ---- 1 ------------------------------------------------------------------------------------------
def test_a_batch_of_one_is_the_single_gather_call(engine, wvb, oracle):
    """Stream and records of hdfs_wirev_fused_compose_packets, downloaded, and the oracle's."""
    from hadoofus_amd import wirev_fused
    a = None
    for k, n in enumerate((0, 1, 1100, N2)):
        lens = [n] if n < 2 else [n // 3, 0, n // 2 - n // 3, n - n // 2]
        for off in (0, 4321):
            for finish in (0, 1):
                s = spec(120 + k, lens, off, 7, bool(finish), (3, 9, 14), 5 + k)
                want = wants(oracle, [s])
                a = a or Arena(engine, room(N2 + N2 + 4096, 8))
                writes = lay(a, [s], want)
                wl = len(want[0][0])
                single = wirev_fused.compose_wirev_fused(writes[0]["frags"], writes[0]["wire_ptr"], wl, off, 7, 2, 2,
                                                         bool(finish))
                assert single == (wl, want[0][1])
                a.check([want[0][0]])
                run(wvb, a, [s], want)


# ---- 2 ------------------------------------------------------------------------------------------
def test_a_mixed_batch_of_twelve_writes(engine, wvb, oracle):
    """Sizes 0 (with and without finish) to about 200 KiB in 1 to 7 fragments;
    the fragments sit at every source residue mod 16 and every write has a
    destination residue of its own."""
    sizes = [0, 0, 1, 511, 513, 1100, 65536, N2, 200 * 1024 + 77, 1100, 513, 65536]
    finish = [True, False, True, False, True, True, False, True, True, False, False, True]
    specs, r = [], 0
    for k, n in enumerate(sizes):
        nf = 1 + (k * 3) % 7 if n else (0 if k else 2)
        lens = ([n // nf] * (nf - 1) + [n - n // nf * (nf - 1)]) if nf else []
        mis = tuple((r + i) % 16 for i in range(max(1, nf)))
        r += sum(1 for x in lens if x)
        specs.append(spec(130 + k, lens, 4321 if k % 2 else 0, 10 * k, finish[k], mis, (5 * k + 3) % 16))
    assert r >= 16 and len({s["dst_mis"] for s in specs}) == 12
    assert {len(s["lens"]) for s in specs} >= {1, 2, 4, 7}
    t = totals(wvb, specs)
    assert t["table_entries"] == 11 and t["seamed_rounds"] > 0 and t["seamed_ragged"] > 0
    want = wants(oracle, specs)
    writes = run(wvb, arena_for(engine, specs, want), specs, want)
    assert {p % 16 for w in writes for p, n in w["frags"] if n} == set(range(16))


# ---- 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ones first", "ones last"])
def test_a_write_of_many_fragments_next_to_a_write_of_one(engine, wvb, oracle, order):
    """1 300 one-byte fragments directly ahead of (behind) a one-fragment
    write, on one workgroup and on the product's grid: a wave's fragment hint
    from the first write must not reach the second one's slice."""
    ones = spec(150, [1] * 1300, 4321, 0, True, (0, 3, 2, 1, 7), 9)
    one = spec(151, [70000], 0, 5, True, (5,), 2)
    specs = [ones, one] if order == "ones first" else [one, ones]
    t = totals(wvb, specs)
    assert (t["nfrags"], t["max_frags_per_round"], t["table_entries"]) == (1301, 512, 2)
    want = wants(oracle, specs)
    run(wvb, arena_for(engine, specs, want), specs, want)


def test_a_ragged_seam_ahead_of_a_seamed_short_first_packet(engine, wvb, oracle):
    """The first write's last chunk (shorter than 512 B) spans two fragments;
    the write behind it starts with a short first packet that spans two as
    well.  The ragged chunk is looked up after the next packet's loads have
    moved the wave to the second write."""
    from hadoofus_amd import wirev_fused
    first = spec(152, [65536 + 4096 + 100, 200], 0, 0, False, (3, 11), 6)
    second = spec(153, [100, 187, 5000], 4321, 9, True, (1, 14, 8), 13)
    assert wirev_fused.layout(first["lens"], 0, 2, 2, False)["seamed_ragged"] == 1
    info = wirev_fused.layout(second["lens"], 4321, 2, 2, True)
    assert info["head_bytes"] == 287 and info["seamed_ragged"] == 1
    many = spec(154, [4097] * 40, 0, 3, False, (2, 7, 12), 1)  # and the same behind a write of many fragments
    for specs in ([first, second], [many, first, second]):
        assert totals(wvb, specs)["seamed_ragged"] >= 2
        want = wants(oracle, specs)
        run(wvb, arena_for(engine, specs, want), specs, want)


# ---- 4 ------------------------------------------------------------------------------------------
def test_three_hundred_one_packet_writes(engine, wvb, oracle):
    """300 writes of one packet in three fragments, one of them of one byte."""
    specs = []
    for k in range(300):
        a, b = 1 + (k * 37) % 900, 1 + (k * 11) % 700
        lens = [[a, 1, b], [1, a, b], [a, b, 1]][k % 3]
        specs.append(spec(1000 + k, lens, 512 * (k % 4), k, k % 7 == 0, (k % 16, (k + 5) % 16, (k + 9) % 16), (3 * k) % 16))
    t = totals(wvb, specs)
    assert t["table_entries"] == 300 and t["nfrags"] == 900 and t["npkts"] == 300 + sum(1 for k in range(300) if k % 7 == 0)
    want = wants(oracle, specs)
    run(wvb, arena_for(engine, specs, want), specs, want)


# ---- 5 ------------------------------------------------------------------------------------------
def test_replicas_overlapping_descending_and_shuffled_fragment_lists(engine, wvb, oracle):
    """Two entries with the same fragment list, entries whose fragments share
    bytes with another entry's, a descending and a shuffled list; between them
    entries without fragments and zero-length fragments with NULL bases."""
    x, y = payload(160, 0, 70001), payload(161, 0, 333)
    a = Arena(engine, room(70001 + 333 + 6 * (2 * 70001 + 4000), 12))
    a.begin()
    px, py = a.put(x, 5), a.put(y, 2)
    lists = [
        [(0, 0, 40000), (0, 40000, 30001)],                      # x in two fragments
        [(0, 0, 40000), (0, 40000, 30001)],                      # its replica
        [],                                                      # iovcnt == 0, finish
        [(0, 20000, 50001), None, (1, 0, 333), (0, 0, 50000)],   # shares bytes with both; a NULL fragment
        [None, None],                                            # nothing but NULL fragments, no finish: no packet
        [(1, 300, 33), (1, 200, 100), (0, 100, 4097), (0, 0, 100)],  # descending
        [(0, 5000, 7), (1, 0, 333), (0, 0, 5000), None, (0, 60000, 10001), (1, 5, 1)],  # shuffled
    ]
    fin = [True, False, True, True, False, False, True]
    datas = [np.concatenate([(x, y)[f[0]][f[1]:f[1] + f[2]] for f in l if f] + [np.zeros(0, np.uint8)]) for l in lists]
    want = [expect(oracle, d, 4321 if k % 2 else 0, k, 2, 2, fin[k]) for k, d in enumerate(datas)]
    writes = [dict(frags=[((px, py)[f[0]] + f[1], f[2]) if f else (None, 0) for f in l],
                   wire_ptr=a.wire(max(1, len(w[0])), (7 * k + 1) % 16), wire_cap=len(w[0]),
                   offset_in_block=4321 if k % 2 else 0, seqno=k, finish=fin[k])
              for k, (l, w) in enumerate(zip(lists, want))]
    assert [len(w[1]) for w in want][2] == 1 and [len(w[1]) for w in want][4] == 0
    a.commit()
    assert wvb.compose(writes) == [(len(w[0]), w[1]) for w in want]
    a.check([w[0] for w in want])
    for g in GROUPS:
        a.commit()
        assert wvb.fused_batch_time(writes, 2, 2, wvb.time_groups(g), 1) > 0
        a.check([w[0] for w in want])


# ---- 6 ------------------------------------------------------------------------------------------
_five = {}


@pytest.mark.parametrize("ctype", [2, 1, 0], ids=["crc32c", "crc32", "null"])
@pytest.mark.parametrize("proto", [2, 1])
def test_protocols_and_checksum_types(engine, wvb, oracle, proto, ctype):
    if not _five:
        _five["specs"] = [spec(170, [300, 2 * 65536 + 7, 5001, 3, 65536 + 34], 0, 100, False, (1, 6, 3, 11, 14), 0),
                          spec(171, [], 512, 0, True),
                          spec(172, [100, 187, 613], 4321, 5, True, (9, 2, 15), 7),
                          spec(173, [65536], 0, 1, False, (13,), 10),
                          spec(174, [4097] * 9, 4321, 50, True, (4, 8, 12), 3)]
    specs = _five["specs"]
    t = totals(wvb, specs, proto, ctype)
    assert t["table_entries"] == 5 and t["seamed_rounds"] >= 9 and t["seamed_ragged"] >= 1
    want = wants(oracle, specs, proto, ctype)
    run(wvb, arena_for(engine, specs, want), specs, want, proto, ctype)


# ---- 7 ------------------------------------------------------------------------------------------
def test_nine_mebibytes_in_four_writes(engine, wvb, oracle):
    """About 9 MiB: 2 305 fragments of 4 097 bytes (nearly every round seamed)
    between 107 KiB in five odd fragments, a write of 1 100 bytes and 128 KiB
    in one fragment; on few workgroups each walks many packets across the
    writes."""
    specs = [spec(180, [30011, 7, 60001, 5, 20000], 4321, 0, True, (3, 1, 7, 5, 9), 6),
             spec(181, [4097] * 2305 + [0], 4321, 1000, True, (3, 1, 7, 5, 9), 11),
             spec(182, [1100], 0, 7, False, (15,), 2),
             spec(183, [2 * 65536], 0, 2000, True, (1,), 13)]
    t = totals(wvb, specs)
    assert t["seamed_rounds"] > 2200 and t["rounds"] - t["seamed_rounds"] > 50 and t["max_frags_per_round"] == 3
    assert t["nfrags"] == 5 + 2305 + 1 + 1 and t["npkts"] > 150
    want = wants(oracle, specs)
    run(wvb, arena_for(engine, specs, want), specs, want)


# ---- 8 ------------------------------------------------------------------------------------------
def test_round_trip_through_the_read_side(engine, wvb, oracle):
    specs = [spec(190, [65536 + 1234, 999, 4 * 65536 - 999], 0, 0, True, (5, 2, 3), 11),
             spec(191, [700, 65536, 4000], 4321, 40, True, (9, 1, 6), 4)]
    want = wants(oracle, specs)
    a = arena_for(engine, specs, want)
    writes = run(wvb, a, specs, want, groups=())
    for k, (s, w) in enumerate(zip(writes, want)):
        ref = oracle.verify_packets(w[0].tobytes())
        got = engine.verify_packets(None, dptr=s["wire_ptr"], nbytes=len(w[0]))
        assert got == ref and got[0] == 0 and got[2] == len(w[0]) and len(got[1]) == len(w[1]), k
    # write 0's seam at byte 65536 + 1234: byte 1233 of its packet 1, in that packet's chunk 2; the byte ahead of it flipped
    p1 = want[0][1][1]
    assert p1["data_off"] == 65536
    at = a.wires[0][0] + p1["hdr_off"] + p1["hdr_len"] + 1233
    a.buf.upload(np.array([want[0][0][at - a.wires[0][0]] ^ 0x20], dtype=np.uint8), at)
    rc, got, _ = engine.verify_packets(None, dptr=writes[0]["wire_ptr"], nbytes=len(want[0][0]))
    assert rc == engine.ERR_BAD_CHECKSUM
    assert [(i, p["first_bad"], p["bad_chunks"]) for i, p in enumerate(got) if p["error"]] == [(1, 2, 1)]
    rc, got, _ = engine.verify_packets(None, dptr=writes[1]["wire_ptr"], nbytes=len(want[1][0]))
    assert rc == 0 and not any(p["error"] for p in got)


# ---- 9 ------------------------------------------------------------------------------------------
def test_rejections_write_nothing(engine, wvb, oracle):
    from hadoofus_amd.abi import OutPacket
    specs = [spec(200, [40000, 0, 60000], 0, 0, True, (1, 0, 6), 3), spec(201, [300, 5000], 4321, 9, True, (7, 12), 8)]
    want = wants(oracle, specs)
    a = arena_for(engine, specs, want)
    base = lay(a, specs, want)
    npk = sum(len(w[1]) for w in want)
    lib = wvb.load()
    pk = (OutPacket * npk)()
    before = bytes(pk)
    cnt = ctypes.c_size_t(0)
    host = np.zeros(70000, dtype=np.uint8)
    end = a.buf.ptr + a.buf.nbytes
    f = [[p for p, _ in w["frags"]] for w in base]
    outs = [dict(len=len(s["d"]), wire_len=len(w[0]), npkts=len(w[1]), first_pkt=fp)
            for s, w, fp in zip(specs, want, (0, len(want[0][1])))]

    def call(mods=(), maxp=npk):
        """mods: {(entry, field) or (entry, fragment): value}."""
        writes = [dict(w, frags=list(w["frags"])) for w in base]
        for (k, what), v in dict(mods).items():
            if isinstance(what, int):
                writes[k]["frags"][what] = (v, writes[k]["frags"][what][1])
            else:
                writes[k][what] = v
        arr, keep = wvb.entries(writes)
        cnt.value = 77
        rc = lib.hdfs_wirev_fused_batch_compose(arr, 2, 2, 2, pk, maxp, ctypes.byref(cnt), None)
        return rc, lib.hdfs_wirev_fused_batch_last_error(), [arr[k].out() for k in range(2)]

    K = lambda **kw: {(int(k[1]), (int(k[3:]) if k[3:].isdigit() else k[3:])): v for k, v in kw.items()}  # noqa: E731
    w0 = base[0]["wire_ptr"]
    cases = {
        "a host fragment": (K(e1_1=host.ctypes.data), (b"entry 1", b"fragment 1")),
        "a host fragment ahead of device ones": (K(e0_0=host.ctypes.data), (b"entry 0", b"fragment 0")),
        "a null base with a length": (K(e0_2=None), (b"entry 0", b"fragment 2")),
        "a fragment past its allocation": (K(e1_1=end - 5000 + 1), (b"entry 1", b"fragment 1")),
        "a wire over a fragment of another entry": (K(e1_wire_ptr=f[0][2] + 60000 - 1), (b"entry 1", b"fragment 2 of entry 0")),
        "a wire over a fragment of its own entry": (K(e0_wire_ptr=f[0][0] + 10), (b"entry 0", b"fragment 0 of entry 0")),
        "a fragment over another entry's wire": (K(e1_1=w0 - 5000 + 1), (b"entry 0", b"fragment 1 of entry 1")),
        "a wire over a wire": (K(e1_wire_ptr=w0 + 100), (b"entry 1", b"wire of entry 0")),
        "a wire past its allocation": (K(e1_wire_ptr=end - len(want[1][0]) + 1), (b"entry 1", b"wire")),
        "a host wire": (K(e0_wire_ptr=host.ctypes.data), (b"entry 0", b"wire")),
        "wire_cap one short": (K(e1_wire_cap=len(want[1][0]) - 1), (b"entry 1",)),
        "max_pkts one short": ({}, (b"entry 1",)),
        "mixed NULL wires": (K(e1_wire_ptr=None), (b"entry 1", b"NULL")),
    }
    for name, (kw, texts) in cases.items():
        rc, err, got = call(kw, npk - 1 if name.startswith("max_pkts") else npk)
        assert rc == EINVAL, name
        assert err and all(t in err for t in texts), (name, err)
        assert got == outs and cnt.value == npk, (name, got)
        assert bytes(pk) == before and not host.any(), name
    # workgroups out of range, or a flag bit that means nothing
    ms = ctypes.c_double(0)
    arr, keep = wvb.entries(base)
    for flags in (wvb.time_groups(wvb.MAX_GROUPS + 1), wvb.time_groups(1 << 23), 1, wvb.time_groups(2) | 4):
        assert lib.hdfs_wirev_fused_batch_time(arr, 2, 2, 2, flags, 1, ctypes.byref(ms)) == EINVAL, flags
        assert b"workgroups" in lib.hdfs_wirev_fused_batch_last_error()
    a.check()
    rc, err, got = call()  # and the same arguments, unspoilt, work
    assert rc == 0 and got == outs, err
    a.check([w[0] for w in want])


# ---- 10 -----------------------------------------------------------------------------------------
def _filled_on(engine, wvb, oracle, seed, stream):
    """Fragments filled by a kernel on `stream` (None: the NULL stream) and the
    call right behind it, no synchronisation between the two."""
    lens = [[1 << 20, 8, (1 << 20) + 64], [512 << 10, 256 << 10]]
    specs = [spec(0, l, 4321 * k, k, False, (8,), 13 - k, data=payload(seed + k, 0, sum(l))) for k, l in enumerate(lens)]
    want = wants(oracle, specs)
    a = arena_for(engine, specs, want)
    zeros = [dict(s, d=np.zeros(len(s["d"]), np.uint8)) for s in specs]
    writes = lay(a, zeros, want)
    for k, w in enumerate(writes):
        at = 0
        for p, ln in w["frags"]:
            assert p % 8 == 0 and ln % 8 == 0
            engine.fill_splitmix64(p, ln // 8, seed + k, at // 8, stream)
            at += ln
    assert wvb.compose(writes, stream=stream) == [(len(w[0]), w[1]) for w in want]
    for s, w in zip(specs, writes):
        for (p, ln), piece in zip(w["frags"], cut(s["d"], s["lens"])):
            a.image[p - a.buf.ptr:p - a.buf.ptr + ln] = piece
    a.check([w[0] for w in want])


def test_fragments_filled_on_the_null_stream_just_before(engine, wvb, oracle):
    """The library's stream waits for the NULL stream."""
    _filled_on(engine, wvb, oracle, 212, None)


def test_on_a_stream_of_the_callers(engine, wvb, oracle):
    st = engine.stream_create()
    try:
        _filled_on(engine, wvb, oracle, 214, st)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, wvb, oracle):
    jobs = []
    for seed, off in ((216, 0), (218, 4321)):
        specs = [spec(seed, [100000, 7, 200000 - 7], off, 0, True, (seed % 4, 9), seed % 16),
                 spec(seed + 1, [123, 150000], 4321 - off, 3, True, (2, 11), 5)]
        want = wants(oracle, specs)
        a = arena_for(engine, specs, want)
        jobs.append((a, lay(a, specs, want), want))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, writes, want = jobs[i]
            start.wait()
            for _ in range(4):
                assert wvb.compose(writes) == [(len(w[0]), w[1]) for w in want]
        except BaseException as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for a, _, want in jobs:
        a.check([w[0] for w in want])


# ---- 11 -----------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "wirev_fused_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wirev_fused_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wirev_fused_batch", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
