/*
 * hadoofus_wire.h -- a write's outgoing packets as one wire stream in device
 * memory (libhadoofus_wire.so, a companion of libhadoofus_crc32c.so built from
 * hadoofus_amd/csrc/wire*).
 *
 * hdfs_crc32c_compose_packets returns the header buffers of a write's packets
 * in host memory and leaves the data where it was: the reference writev()s
 * the two (src/datanode.c:2781-2868).  The read side of the main library takes
 * the packets as the wire carries them, one contiguous run
 * [plen][hlen][PacketHeaderProto][BE CRCs][data]... in device memory
 * (hdfs_crc32c_verify_packets, hdfs_crc32c_read_packets, jobs, readers).
 * This library produces that run on the device from a write that lives there:
 * for a device-to-device replica hop, a send straight from device memory, or
 * one contiguous copy to the host followed by one write().
 *
 * The chunk CRCs come from one compute plan of the main library over
 * hdfs_crc32c_compose_packets' chunk grid (no CRC arithmetic here); this
 * library's own kernel, frame_packets_kernel, then writes every byte of the
 * stream once: the headers it composes itself from the packet index, the CRCs
 * from the plan's array, the data from the caller's buffer.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.
 *
 * WHEN IT PAYS.  Without this library a caller gets the same stream from
 * hdfs_crc32c_compose_packets on the device buffer, one host-to-device copy of
 * the header buffers and two hipMemcpyAsync device-to-device per packet into
 * a stream allocated beforehand.  Measured on one MI355X
 * (tools/wire_bench.py; medians of 5 with the two paths
 * alternated in one process, host clock around each whole path, CRC32C, v2,
 * finish, source at an odd address, both paths' bytes compared):
 *     write     block offset   this call    copies (of it: issuing them)
 *     128 MiB        0          0.18 ms      13.3 ms   (13.1)
 *     128 MiB     4321          0.20 ms      12.9 ms   (12.6)
 *       1 GiB        0          0.79 ms     101.2 ms  (100.1)
 *       1 GiB     4321          0.85 ms     102.3 ms  (101.1)
 * The copies cost about 3.1 us of host time each (4 097 of them for 128 MiB,
 * the interpreter's loop, 0.35 ms, taken off), as DESIGN section 12 found for
 * gather writes; this call was 65 to 130 times faster and the copies won
 * nowhere.  Another run of the same command gave 0.21 / 0.22 / 0.80 / 0.81 ms
 * for this call.  The frame kernel alone (HIP events around ten back-to-back
 * launches) took 0.046 ms for 128 MiB and 0.425 ms for 1 GiB: 5.8 and 5.1 TB/s
 * of traffic (len + 4 B per chunk read, the stream written), beside the 5.1 TB/s
 * recorded for copy_pieces_kernel; the 128 MiB figure is
 * helped by the last-level cache, which holds most of that write.  A 128 MiB
 * call is therefore mostly fixed cost (the plan's creation, two launches, the
 * synchronise), not the time the bytes take.  Writes below 128 MiB were not
 * measured against the copies.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_wire_last_error()).
 */
#ifndef HADOOFUS_WIRE_H
#define HADOOFUS_WIRE_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_WIRE_<n>
 * (hadoofus_amd/csrc/wire_exports.map); run-time bindings compare
 * hdfs_wire_abi_version() with the version they were written for.  The main
 * library's ABI version is not affected by this one. */
#define HDFS_WIRE_ABI_VERSION 1

int hdfs_wire_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_wire_last_error(void);

/* The packets of one write of len bytes at `data`, as one stream at `wire`:
 * after a successful call wire[0, *wire_len) is, packet after packet, the
 * packet's header buffer exactly as hdfs_crc32c_compose_packets writes it
 * (plen, then hlen + PacketHeaderProto (v2) or the 25-byte v1 header, then the
 * BE chunk CRCs) followed by the packet's data_len bytes of `data`.  Packet
 * sizing, finish, proto, ctype, offset_in_block and seqno are
 * hdfs_crc32c_compose_packets': the short first packet that completes an
 * unaligned block offset's chunk and the empty lastPacketInBlock packet of
 * `finish` included.  HDFS_CRC32C_CSUM_NULL gives headers and data with no
 * CRC bytes.  The records in pkts (may be NULL) equal
 * hdfs_crc32c_compose_packets' field for field, except that hdr_off is the
 * offset of the packet's first byte in `wire`: packet i's data lies at
 * hdr_off + hdr_len, packet i + 1 at hdr_off + hdr_len + data_len.
 *
 * data and wire are device memory of the engine's device at any byte
 * alignment, each range inside one device allocation, the two not overlapping;
 * host pointers, a range that leaves its allocation, overlapping ranges,
 * wire_cap < *wire_len and (with pkts) max_pkts < *npkts are
 * HDFS_CRC32C_EINVAL with nothing written, *npkts and *wire_len still set.
 * wire == NULL is a size query that touches no device: *npkts and *wire_len
 * are set, and the records too when pkts has room (they follow from the
 * arguments alone).  An empty write with finish is one header-only packet; an
 * empty write without it is no packet and no work.  At most 1 TiB per call.
 *
 * Only [data, data + len) is read and only [wire, wire + *wire_len) is
 * written, every byte of it once.
 *
 * ORDERING.  The work (the plan, then the frame kernel) is enqueued on
 * `stream`, a hipStream_t of the engine's device; NULL is a stream of this
 * library that waits for the NULL stream (a blocking stream): bytes written
 * by other non-blocking streams must then be complete before the call.  With a
 * stream of the caller's, the data must be ordered ahead of the call on that
 * stream.  The call returns after the stream has been synchronised: the
 * stream's bytes are then visible to every later operation on the device.
 * Calls from several threads are serialised inside the library (one CRC array,
 * grown on demand and kept). */
int hdfs_wire_compose_packets(const void *data, uint64_t len, int64_t offset_in_block, int64_t seqno,
    int proto, int ctype, int finish, void *wire, uint64_t wire_cap, hdfs_crc32c_out_packet *pkts,
    size_t max_pkts, size_t *npkts, uint64_t *wire_len, void *stream);

/* Host only, no GPU: the shape of the stream of such a write. */
typedef struct hdfs_wire_layout_info {
	uint64_t npkts;          /* packets, the empty last one of `finish` included */
	uint64_t nchunks;        /* chunks on the write's chunk grid (CRCs computed unless CSUM_NULL) */
	uint64_t wire_len;       /* bytes of the stream */
	uint32_t packet_stride;  /* bytes of a full 64 KiB packet: 66 079 (v2) / 66 073 (v1) with checksums */
	uint32_t header_bytes;   /* bytes ahead of a packet's CRCs: 31 (v2) / 25 (v1) */
	uint32_t head_bytes;     /* data bytes of the short first packet (0: none) */
	uint32_t reserved;
} hdfs_wire_layout_info;
int hdfs_wire_layout(uint64_t len, int64_t offset_in_block, int proto, int ctype, int finish,
    hdfs_wire_layout_info *out);

/* Measurement (tools/wire_bench.py): hdfs_wire_compose_packets once, then the
 * frame kernel alone iters more times on the library's stream between two HIP
 * events; *ms_per_iter is their distance over iters.  flags: HDFS_WIRE_TIME_SC1
 * makes the 16-B stores write-through, HDFS_WIRE_TIME_SLICES(n) deals a
 * packet to n workgroups (1..16) instead of the product's choice.  The stream
 * written is the same under every flag. */
#define HDFS_WIRE_TIME_SC1 1u
#define HDFS_WIRE_TIME_SLICES(n) ((unsigned)(n) << 8)
int hdfs_wire_frame_time(const void *data, uint64_t len, int64_t offset_in_block, int proto, int ctype,
    int finish, void *wire, uint64_t wire_cap, unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_WIRE_H */
