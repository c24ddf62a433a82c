/*
 * hadoofus_wirev.h -- a write held in a list of device buffers as one wire
 * stream in device memory (libhadoofus_wirev.so, a companion of
 * libhadoofus_crc32c.so built from hadoofus_amd/csrc/wirev*).
 *
 * The reference's write entry points take an iovec array
 * (hdfs_datanode_writev / hdfs_datanode_writev_nb, include/lowlevel.h:627,
 * 853) and chain every 512-B chunk's CRC across fragment boundaries
 * (src/datanode.c:2836-2859).  hadoofus_writev.h composes such a write's
 * packets from device fragments but stops at header buffers in host memory;
 * hadoofus_wire.h writes the whole stream
 * [plen][hlen][PacketHeaderProto][BE CRCs][data]... in device memory, the
 * bytes the read side consumes (hdfs_crc32c_verify_packets,
 * hdfs_crc32c_read_packets, jobs, readers), but takes one contiguous source.
 * This library joins the two: device fragments in, one device stream out,
 * without packing the fragments into a second allocation first.
 *
 * The chunk CRCs are computed as hadoofus_writev.h computes them (runs of
 * whole chunks inside one fragment as segments of one compute plan of the
 * main library, the other chunks piece by piece by gather_chunks_kernel) and
 * stay on the device; this library's own kernel, frame_gather_kernel, then
 * writes every byte of the stream once: the headers it composes itself, the
 * CRCs from that array, the data from the fragments, found through a table
 * of where each fragment starts in the write.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  The alternative is packing: one hipMemcpyAsync
 * device-to-device per fragment into a contiguous buffer (a second
 * allocation of the write's size), then hdfs_wire_compose_packets on it.
 * Measured on one MI355X (tools/wirev_bench.py; medians
 * of 5 with the two paths alternated in one process, host clock around each
 * whole path, CRC32C, v2, finish, fragments at odd addresses, the packed buffer
 * allocated beforehand, both paths' bytes compared):
 *     write      fragments          block offset   in place     packed (of it: issuing the copies)
 *     128 MiB        1                    0         0.15 ms      0.24 ms  (0.003)
 *     128 MiB        1                 4321         0.19 ms      0.26 ms  (0.006)
 *     128 MiB       16 x 8 MiB         4321         0.21 ms      0.30 ms  (0.06)
 *     128 MiB      128 x 1 MiB         4321         0.25 ms      0.62 ms  (0.43)
 *     128 MiB    1 024 x 128 KiB       4321         0.42 ms      3.60 ms  (3.35)
 *     128 MiB   16 383 x 8 193 B       4321         4.25 ms     55.7 ms  (51.3)
 *     128 MiB   33 555 x 4 000 B       4321         7.16 ms    119.2 ms (118.8)
 *       1 GiB       64 x 16 MiB        4321         0.91 ms      1.52 ms  (0.23)
 * In place was faster at every shape measured, block offset 0 included (there
 * 0.15 to 7.3 ms): there is no fragment size down to 4 000 B at which packing
 * wins, because packing costs about 3.4 us of host time per copy issued.  The
 * frame kernel alone runs at the contiguous library's rate with one fragment
 * (46.4 us, 5.8 TB/s of traffic for 128 MiB), within 16 % of it down to
 * 128 KiB fragments, at 2.8 TB/s with 8 193 B and 1.85 TB/s with 4 000 B
 * fragments; calls with thousands of small fragments are dominated by the
 * gather-write library's costs (layout, tables, one lane per gathered chunk,
 * hadoofus_writev.h), not by framing.  With a single fragment the call costs
 * what hdfs_wire_compose_packets costs at an aligned block offset (0.151
 * against 0.149 ms) and 27 us more at an unaligned one (0.191 against
 * 0.164 ms: the short first chunk is gathered, two small table uploads and a
 * kernel launch).  Writes below 128 MiB and fragments below 4 000 B were not
 * measured.
 *
 * A workgroup of the frame kernel walks the fragments under its packet one
 * after the other, one scalar round trip per piece: a packet made of tens of
 * thousands of one-byte fragments is framed correctly but slowly.  There is no
 * second mapping for such writes.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_wirev_last_error()).
 */
#ifndef HADOOFUS_WIREV_H
#define HADOOFUS_WIREV_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_WIREV_<n>
 * (hadoofus_amd/csrc/wirev_exports.map); run-time bindings compare
 * hdfs_wirev_abi_version() with the version they were written for.  The main
 * library's ABI version is not affected by this one. */
#define HDFS_WIREV_ABI_VERSION 1

int hdfs_wirev_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_wirev_last_error(void);

/* hdfs_wire_compose_packets for a write held in iovcnt fragments: after a
 * successful call wire[0, *wire_len) is byte for byte what
 * hdfs_wire_compose_packets writes for the fragments' concatenation, and the
 * records in pkts (may be NULL) are that call's: hdr_off counts in the
 * stream, data_off in the concatenation.  Packet sizing, finish, proto,
 * ctype, offset_in_block and seqno are hdfs_crc32c_compose_packets'.
 * HDFS_CRC32C_CSUM_NULL does no CRC work and still frames headers and data.
 *
 * Fragments are device memory of the engine's device, each inside one device
 * allocation, at any byte alignment and of any length; zero-length fragments
 * are allowed anywhere (base may then be NULL); fragments may overlap each
 * other, come in any address order and repeat.  wire is device memory of the
 * same device, [wire, wire + *wire_len) inside one allocation and clear of
 * every fragment.  A host or mixed fragment list, a fragment that runs past
 * its allocation, a wire range outside one allocation or over a fragment,
 * wire_cap < *wire_len and (with pkts) max_pkts < *npkts are
 * HDFS_CRC32C_EINVAL with nothing written, *npkts and *wire_len still set;
 * the text names the fragment.  wire == NULL is a size query that touches no
 * device and reads only the fragments' lengths: *npkts and *wire_len are set,
 * and the records too when pkts has room.  An empty write with finish is one
 * header-only packet; an empty write without it is no packet and no work.  At
 * most 1 TiB per call.
 *
 * Only the fragments are read, and only inside the aligned 4-byte words that
 * hold their bytes; only [wire, wire + *wire_len) is written, every byte of
 * it once.
 *
 * ORDERING.  As hdfs_wire_compose_packets: the work (the fragment table's
 * upload, the CRCs, then the frame kernel) is enqueued on `stream`, a
 * hipStream_t of the engine's device; NULL is a stream of this library that
 * waits for the NULL stream (a blocking stream).  With a stream of the
 * caller's, the fragments' bytes must be ordered ahead of the call on that
 * stream.  The call returns after the stream has been synchronised.  Calls
 * from several threads are serialised inside the library, from the table
 * upload to that synchronise (one set of tables and one CRC array, grown on
 * demand and kept). */
int hdfs_wirev_compose_packets(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block, int64_t seqno,
    int proto, int ctype, int finish, void *wire, uint64_t wire_cap, hdfs_crc32c_out_packet *pkts,
    size_t max_pkts, size_t *npkts, uint64_t *wire_len, void *stream);

/* Host only, no GPU: the shape of the stream of a write of these fragment
 * lengths and how its chunk grid is split over the fragments: what
 * hdfs_wire_layout reports for the total length and what hdfs_writev_layout
 * reports for the lengths, and the fragment table's size. */
typedef struct hdfs_wirev_layout_info {
	uint64_t npkts;          /* packets, the empty last one of `finish` included */
	uint64_t nchunks;        /* chunks on the write's chunk grid (CRCs computed unless CSUM_NULL) */
	uint64_t wire_len;       /* bytes of the stream */
	uint64_t nsegments;      /* in-place segments of the compute plan */
	uint64_t seg_chunks;     /* the chunks they cover */
	uint64_t ngathered;      /* chunks assembled from pieces */
	uint64_t npieces;        /* their pieces */
	uint64_t nfrags;         /* non-empty fragments: entries of the frame kernel's table */
	uint32_t packet_stride;  /* bytes of a full 64 KiB packet: 66 079 (v2) / 66 073 (v1) with checksums */
	uint32_t header_bytes;   /* bytes ahead of a packet's CRCs: 31 (v2) / 25 (v1) */
	uint32_t head_bytes;     /* data bytes of the short first packet (0: none) */
	uint32_t max_pieces;     /* most pieces in one gathered chunk */
	uint32_t max_frags_per_packet; /* most non-empty fragments under one packet's data */
	uint32_t reserved;
} hdfs_wirev_layout_info;
int hdfs_wirev_layout(const uint64_t *lens, int iovcnt, int64_t offset_in_block, int proto, int ctype, int finish,
    hdfs_wirev_layout_info *out);

/* Measurement (tools/wirev_bench.py): hdfs_wirev_compose_packets once, then
 * the frame kernel alone iters more times on the library's stream between two
 * HIP events; *ms_per_iter is their distance over iters.  flags as
 * hdfs_wire_frame_time's: HDFS_WIREV_TIME_SC1 makes the 16-B stores
 * write-through, HDFS_WIREV_TIME_SLICES(n) deals a packet to n workgroups
 * (1..16) instead of the product's four.  The stream written is the same
 * under every flag. */
#define HDFS_WIREV_TIME_SC1 1u
#define HDFS_WIREV_TIME_SLICES(n) ((unsigned)(n) << 8)
int hdfs_wirev_frame_time(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block, int proto, int ctype,
    int finish, void *wire, uint64_t wire_cap, unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_WIREV_H */
