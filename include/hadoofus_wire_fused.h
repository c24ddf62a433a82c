/*
 * hadoofus_wire_fused.h -- a write's outgoing packets as one wire stream in
 * device memory, in ONE pass over the data (libhadoofus_wire_fused.so, a
 * companion of libhadoofus_crc32c.so built from hadoofus_amd/csrc/wire_fused*).
 *
 * hdfs_wire_compose_packets (hadoofus_wire.h) makes the stream in two passes:
 * a compute plan of the main library reads the write and leaves the chunk CRCs
 * in a scratch array, then a frame kernel reads the write again and writes the
 * stream.  This library's kernel, frame_fused_kernel, reads the write once:
 * the registers it loads go straight out to the packet's data region, the
 * chunk CRCs are computed from those registers and stored into the packet's
 * CRC region by the lanes that hold them, and the headers are composed from
 * the packet index.  There is no compute plan, no CRC array and one launch.
 * The price is a second implementation of the CRC arithmetic (the slicing
 * step and the in-register transpose of the main library's tiled kernel),
 * built from the same table code (crc32c_tables.h).
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  At every size measured, against hdfs_wire_compose_packets
 * on the same arguments.  One MI355X (tools/wire_fused_bench.py, DESIGN.md
 * section 16; medians of 5 (min-max) with the two calls alternated in one
 * process after one warm-up of each, host clock around each whole call, which
 * ends in its synchronise, CRC32C, v2, finish, source at an odd address, all
 * buffers allocated beforehand, both streams downloaded and compared):
 *     write     block offset   this call (min-max)        two-pass call (min-max)
 *       1 MiB        0      0.026 ms (0.025-0.040)      0.061 ms (0.060-0.069)
 *       1 MiB     4321      0.024 ms (0.023-0.024)      0.077 ms (0.076-0.078)
 *       8 MiB        0      0.028 ms (0.027-0.028)      0.065 ms (0.064-0.065)
 *       8 MiB     4321      0.026 ms (0.026-0.027)      0.084 ms (0.082-0.084)
 *     128 MiB        0      0.102 ms (0.099-0.107)      0.149 ms (0.148-0.153)
 *     128 MiB     4321      0.081 ms (0.081-0.086)      0.159 ms (0.154-0.161)
 *       1 GiB        0      0.656 ms (0.651-0.660)      0.735 ms (0.729-0.739)
 *       1 GiB     4321      0.647 ms (0.641-0.659)      0.757 ms (0.751-0.769)
 * The two ranges are clear of each other in all eight rows, and were in an
 * earlier run of the same command.  Up to 8 MiB the win (2.3 to 3.2 times) is
 * fixed cost: no plan is created or destroyed and there is one launch.  At
 * 128 MiB (1.5 to 2.0 times) it is both fixed cost and GPU time.  At 1 GiB
 * (1.12 to 1.17 times) it is GPU time alone, and smaller than the pass saved:
 * the fused kernel alone (HIP events around ten back-to-back launches) took
 * 0.503 / 0.485 ms for the gigabyte, 4.3 to 4.5 TB/s of traffic (len read, the
 * stream written), where the two-pass library's frame kernel took 0.412 ms
 * after a plan of 0.171 to 0.185 ms: the copy under the CRC is 17 to 22 %
 * slower than the plain copy, mostly, it seems, for its unaligned 16-byte
 * accesses.  Below 128 MiB the fused kernel alone (12 to 14 us) is slower than
 * the frame kernel alone (4 to 6 us): every workgroup fills 156 KiB of tables
 * before its first load.  Not measured: CRC32, v1, CSUM_NULL, a caller's
 * stream, sizes between 8 and 128 MiB and above 1 GiB.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_wire_fused_last_error()).
 */
#ifndef HADOOFUS_WIRE_FUSED_H
#define HADOOFUS_WIRE_FUSED_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_WIRE_FUSED_<n>
 * (hadoofus_amd/csrc/wire_fused_exports.map); run-time bindings compare
 * hdfs_wire_fused_abi_version() with the version they were written for.  The
 * main library's ABI version is not affected by this one. */
#define HDFS_WIRE_FUSED_ABI_VERSION 1

int hdfs_wire_fused_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_wire_fused_last_error(void);

/* Same arguments, same contract, same records, same bytes as
 * hdfs_wire_compose_packets (hadoofus_wire.h).  The packets of one write of
 * len bytes at `data`, as one stream at `wire`: after a successful call
 * wire[0, *wire_len) is byte for byte that call's stream -- packet after
 * packet, the header buffer exactly as hdfs_crc32c_compose_packets writes it
 * (plen, then hlen + PacketHeaderProto (v2) or the 25-byte v1 header, then the
 * BE chunk CRCs) followed by the packet's data_len bytes of `data`, the short
 * first packet that completes an unaligned block offset's chunk and the empty
 * lastPacketInBlock packet of `finish` included.  HDFS_CRC32C_CSUM_NULL gives
 * headers and data with no CRC bytes.  The records in pkts (may be NULL) are
 * that call's: hdr_off is the offset of the packet's first byte in `wire`.
 *
 * data and wire are device memory of the engine's device at any byte
 * alignment, each range inside one device allocation, the two not overlapping;
 * host pointers, a range that leaves its allocation, overlapping ranges,
 * wire_cap < *wire_len and (with pkts) max_pkts < *npkts are
 * HDFS_CRC32C_EINVAL with nothing written, *npkts and *wire_len still set.
 * wire == NULL is a size query that touches no device: *npkts and *wire_len
 * are set, and the records too when pkts has room.  An empty write with finish
 * is one header-only packet; an empty write without it is no packet and no
 * work.  At most 1 TiB per call.
 *
 * Only [data, data + len) is read and only [wire, wire + *wire_len) is
 * written, every byte of it once.
 *
 * ORDERING.  The kernel is enqueued on `stream`, a hipStream_t of the engine's
 * device; NULL is a stream of this library that waits for the NULL stream (a
 * blocking stream): bytes written by other non-blocking streams must then be
 * complete before the call.  With a stream of the caller's, the data must be
 * ordered ahead of the call on that stream.  The call returns after the stream
 * has been synchronised: the stream's bytes are then visible to every later
 * operation on the device.  Calls from several threads are serialised inside
 * the library by one mutex (the tables, uploaded once per device and kept). */
int hdfs_wire_fused_compose_packets(const void *data, uint64_t len, int64_t offset_in_block, int64_t seqno,
    int proto, int ctype, int finish, void *wire, uint64_t wire_cap, hdfs_crc32c_out_packet *pkts,
    size_t max_pkts, size_t *npkts, uint64_t *wire_len, void *stream);

/* Measurement (tools/wire_fused_bench.py): hdfs_wire_fused_compose_packets
 * once, then the fused kernel alone iters more times on the library's stream
 * between two HIP events; *ms_per_iter is their distance over iters.  flags:
 * HDFS_WIRE_FUSED_TIME_GROUPS(n) launches n workgroups (1..1024) instead of
 * the product's grid (one per compute unit, at most one per packet), so that
 * every workgroup walks many packets; any other flag bit, or n above 1024, is
 * HDFS_CRC32C_EINVAL with nothing written.  The stream written is the same
 * under every flag. */
#define HDFS_WIRE_FUSED_TIME_GROUPS(n) ((unsigned)(n) << 8)
int hdfs_wire_fused_time(const void *data, uint64_t len, int64_t offset_in_block, int proto, int ctype,
    int finish, void *wire, uint64_t wire_cap, unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_WIRE_FUSED_H */
