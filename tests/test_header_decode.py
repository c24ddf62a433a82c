"""PacketHeaderProto decoding: frame::decode_header (crc32c_frame.h) on the
host walk against the oracle's pb_header (oracle/crc32c_oracle.c) and against
what each header was BUILT to mean (packet_stream.random_header: the expected
decode comes from the construction, no decoder involved).

The reference unpacks the header with protobuf-c (src/datanode.c:2387-2418),
which it takes from the system: it ships no copy, and no protobuf-c is
available to build against here, so the rules are pinned by construction and,
where google.protobuf imports, by google.protobuf's parser.  The two parsers
differ in one documented place: a known field number carrying another wire
type is a rejection for protobuf-c (its scan fails the message), while
google.protobuf keeps such a field as an unknown one and goes on.  Draws with
that defect are left out of the google.protobuf comparison for that reason;
everything else must agree with it.
"""
import struct

import numpy as np
import pytest

from packet_stream import (REJECT_REASONS, frame_v2, header_class, header_v2, header_v2_padded, header_v2_variant,
                           random_header)

ERR_PROTO, ERR_SIZE = 18, 25
DRAWS, SEED = 5000, 20240607


def _s32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _expect(hdr, fields):
    """What the walk gives [plen = 4][hlen][hdr], one packet without CRCs or
    data, when hdr decodes to `fields` (None: rejected) -- from
    _process_recv_packet's checks (src/datanode.c:2428-2456): crcdlen =
    plen - dataLen - 4 = -dataLen, so dataLen != 0 is PACKET_SIZE with the
    decoded fields recorded, and dataLen 0 is the empty last packet (PACKET_SIZE
    when it is not flagged last).  -> (rc, [record], consumed)."""
    rec = {"stream_off": 0, "offset_in_block": 0, "seqno": 0, "data_len": 0, "crc_len": 0, "header_len": 6 + len(hdr),
           "error": ERR_PROTO, "first_bad": -1, "bad_chunks": 0, "last": 0, "sync": 0}
    if fields is not None:
        off, seq, last, dlen, sync = fields
        err = ERR_SIZE if (dlen != 0 or not last) else 0
        rec.update(offset_in_block=off, seqno=seq, data_len=dlen, crc_len=_s32(-dlen), error=err, last=int(last),
                   sync=int(sync))
    return rec["error"], [rec], 0 if rec["error"] else 6 + len(hdr)


def test_random_headers_engine_oracle_construction(oracle):
    """5 000 seeded encodings -- reordered, repeated, padded, unknown fields,
    long bools, and every way protobuf-c's scan fails -- each framed as one
    packet: the engine's host walk, the oracle and the construction agree on
    the fields and header_len, or on INVALID_PACKETHEADERPROTO with nothing
    consumed.  The mix of draws is asserted, so the generator cannot go
    degenerate; the counts are taken from the oracle's verdicts as well."""
    import hadoofus_amd as h
    try:
        PH = header_class()
    except ImportError:
        PH = None
    rng = np.random.default_rng(SEED)
    accepted = oracle_accepted = compared = 0
    reasons = dict.fromkeys(REJECT_REASONS, 0)
    for i in range(DRAWS):
        info = {}
        hdr, fields = random_header(rng, info)
        assert len(hdr) <= 0xFFFF
        s = frame_v2(hdr, b"", b"", plen=4)
        want = _expect(hdr, fields)
        got_o = oracle.verify_packets(s, max_pkts=4)
        got_e = h.parse_packets(s, max_pkts=4)
        assert got_o == want, (i, info, hdr.hex())
        assert got_e == want, (i, info, hdr.hex())
        oracle_accepted += got_o[1][0]["error"] != ERR_PROTO
        if fields is not None:
            accepted += 1
            assert info["reason"] is None
        else:
            reasons[info["reason"]] += 1
        if PH is not None and info["reason"] != "wire_type":
            compared += 1
            m = PH()
            try:
                m.ParseFromString(hdr)
                ok = m.IsInitialized()
            except Exception as e:
                assert type(e).__name__ == "DecodeError", e
                ok = False
            assert ok == (fields is not None), (i, info, hdr.hex())
            if ok:
                assert (m.offsetInBlock, m.seqno, m.lastPacketInBlock, m.dataLen, m.syncBlock) == fields
    assert accepted >= DRAWS // 4 and DRAWS - accepted >= DRAWS // 4, accepted
    assert oracle_accepted == accepted
    assert min(reasons.values()) >= 100, reasons
    assert PH is None or compared >= DRAWS * 3 // 4


@pytest.mark.parametrize("total", [63, 64, 65, 4000, 65541])
@pytest.mark.parametrize("front", [True, False], ids=["pad_first", "pad_last"])
def test_header_lengths_at_the_window(oracle, total, front):
    """Headers of exactly 63 / 64 / 65 wire bytes (one below, at and one above
    the 64-byte header window), 4 000 and 65 541 (hlen = 65 535, the largest
    the u16 holds): the known fields before or behind an unknown bytes field
    that makes up the length."""
    import hadoofus_amd as h
    off, seq, last, dlen, sync = 3 * 65536, 3, True, 0, None
    hdr = header_v2_padded(total, off, seq, last, dlen, sync, front=front)
    assert 6 + len(hdr) == total
    s = frame_v2(hdr, b"", b"", plen=4)
    assert struct.unpack(">H", s[4:6])[0] == total - 6
    want = _expect(hdr, (off, seq, last, dlen, False))
    assert oracle.verify_packets(s, max_pkts=4) == want
    assert h.parse_packets(s, max_pkts=4) == want
    # one byte short of the header: incomplete, nothing recorded
    assert oracle.verify_packets(s[:-1], max_pkts=4) == (0, [], 0)
    assert h.parse_packets(s[:-1], max_pkts=4) == (0, [], 0)


def test_variant_builder_means_what_it_says(oracle):
    """header_v2_variant's knobs, one at a time and together, decode to the
    fields they were given (the encodings the GPU tests run at scale)."""
    import hadoofus_amd as h
    f = (7 * 65536, 7, False, 0, True)
    kws = [dict(), dict(order=(4, 3, 2, 1, 5)), dict(order=(5, 4, 3, 2, 1)), dict(repeat=1), dict(repeat=4),
           dict(repeat=3), dict(repeat=5), dict(tag_pad=4), dict(bool_bytes=10), dict(bool_bytes=2),
           dict(unknown=((4, 6, 0, 1),)), dict(unknown=((0, 6, 2, 31), (2, 1000, 1, 5), (9, (1 << 29) - 1, 5, 6))),
           dict(order=(3, 1, 5, 4, 2), repeat=2, tag_pad=2, bool_bytes=7,
                unknown=((1, 77, 2, 200), (3, 9, 0, 1 << 40)))]
    seen = set()
    for kw in kws:
        hdr = header_v2_variant(*f, **kw)
        assert (hdr == header_v2(*f)) == (not kw)
        seen.add(hdr)
        s = frame_v2(hdr, b"", b"", plen=4)
        want = _expect(hdr, f)
        assert oracle.verify_packets(s, max_pkts=4) == want, kw
        assert h.parse_packets(s, max_pkts=4) == want, kw
    assert len(seen) == len(kws)
