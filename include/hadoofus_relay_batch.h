/*
 * hadoofus_relay_batch.h -- a batch of verified reads re-framed as writes in
 * one call: the packet streams of many block transfers, all in device memory,
 * are verified and their payload is written out again as the packet streams of
 * writes to another datanode, by one launch, one pass over the bytes and one
 * synchronise (libhadoofus_relay_batch.so, a companion of libhadoofus_crc32c.so
 * built from hadoofus_amd/csrc/relay_batch*).
 *
 * A client's most common bulk job uses both ends of the data path: a block is
 * read from one datanode and written to another (distcp, and every "copy this
 * file" above hdfs_datanode_read + hdfs_datanode_write).  With the libraries
 * beside this one that is two calls with a buffer between them:
 * hdfs_read_batch_read_blocks loads the stream, verifies it and stores the
 * payload; hdfs_wire_fused_batch_compose loads the payload again, computes once
 * more exactly the CRCs the first call just verified, and stores the new
 * stream.  That is about four bytes of memory traffic per payload byte, two
 * table uploads, two synchronises and a payload-sized buffer.  Both kernels run
 * the same round, one the reverse of the other, and a read stream's chunk grid
 * is the write's chunk grid whenever the write starts on a chunk boundary: so
 * the CRC computed from the registers of ONE load serves both, compared with
 * the input's CRC bytes and stored as the output's.  What differs is the
 * framing.  The headers are composed anew (the writer's offsetInBlock, seqno
 * and lastPacketInBlock), and the packets are cut anew: a datanode sends what
 * it likes (stock HDFS: 126 chunks = 64512 B a packet), the writer sends
 * PACKET_SIZE = 65536 B (src/datanode.c:2590).
 *
 * An entry whose input is not of the regular shape (hadoofus_read_batch.h), or
 * whose write does not start on the 512-B chunk grid, or in which the launch
 * met a header or a CRC that is not the expected one, is served inside the call
 * by hdfs_crc32c_read_packets into a buffer of the library's and the fused
 * framing kernel over it (path = HDFS_RELAY_BATCH_PATH_FALLBACK).  No entry's
 * result depends on which path it took.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  At every shape measured, against
 * hdfs_read_batch_read_blocks into a preallocated buffer (no records) followed
 * by hdfs_wire_fused_batch_compose of it (no records).  One MI355X
 * (tools/relay_batch_bench.py, profiles/relay_batch_bench.json, DESIGN.md
 * section 25; medians of 5 (min-max) per entry with the two paths alternated
 * in one process after a warm-up of each, host clock around each whole path,
 * which ends in its synchronise, CRC32C, v2, input streams with the empty last
 * packet at odd addresses, writes at offset 512 with finish, every byte of both
 * outputs compared on the device), microseconds per entry:
 *     entries x size, input packets    this call           the two calls          launches alone
 *      16 x 128 MiB, 65536 B           68.9 (67.7-70.9)    143.2 (142.2-151.4)    65.9
 *      16 x 128 MiB, 64512 B           67.2 (67.0-67.8)    140.5 (139.2-143.1)    65.3
 *      64 x 128 MiB, 65536 B           66.4 (66.4-70.0)    140.1 (139.7-140.8)    65.4
 *      64 x 128 MiB, 64512 B           64.8 (64.5-66.5)    136.2 (135.8-137.0)    63.8
 *      64 x 128 MiB, 64512 B, 1 bad    66.9 (66.2-69.7)    137.8 (137.6-138.7)    63.9
 *      64 x   1 MiB, 64512 B           1.52 (1.51-1.58)    2.47 (2.45-2.60)       1.04
 *     256 x  64 KiB, 64512 B           0.59 (0.56-0.60)    0.74 (0.72-0.80)       0.23
 * This call's range is clear of the two calls' in all seven rows: 2.1 times
 * for 128 MiB entries, where it moves half the bytes (4.1 to 4.2 TB/s of stream
 * read plus stream written in the launches alone) and costs what
 * hdfs_read_batch_read_blocks alone costs (hadoofus_read_batch.h: 72.6 to 74.2
 * us), 1.6 times for 1 MiB entries and 1.3 times for 64 KiB entries, where the
 * fixed cost of a call dominates both.  Stock HDFS's 64512-byte input packets,
 * whose rounds cross packet seams, cost no more than 65536-byte ones.  One
 * corrupt entry of 64 (the fifth row) costs the call one
 * hdfs_crc32c_read_packets of that entry.  Where it is weak: a write off the
 * 512-B chunk grid and an irregular input take the fallback, which is slower
 * than the two calls batched (one entry at a time, a synchronise each).  Not
 * measured: CRC32, v1, a caller's stream, many fallbacks in one batch,
 * unaligned writes, input packets below 4 KiB, a second run of the command.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_relay_batch_last_error()).
 */
#ifndef HADOOFUS_RELAY_BATCH_H
#define HADOOFUS_RELAY_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_RELAY_BATCH_<n>
 * (hadoofus_amd/csrc/relay_batch_exports.map); run-time bindings compare
 * hdfs_relay_batch_abi_version() with the version they were written for.  The
 * main library's ABI version and the other companions' are not affected. */
#define HDFS_RELAY_BATCH_ABI_VERSION 1

/* Most entries in one call. */
#define HDFS_RELAY_BATCH_MAX_ENTRIES 1024

#define HDFS_RELAY_BATCH_PATH_KERNEL   0   /* verified and re-framed by this library's launch */
#define HDFS_RELAY_BATCH_PATH_FALLBACK 1   /* hdfs_crc32c_read_packets, then the fused framing kernel, inside the call */

int hdfs_relay_batch_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_relay_batch_last_error(void);

/* One verified read re-framed as one write, and what the call reports back. */
typedef struct hdfs_relay_batch_entry {
	/* in: the read */
	const void *stream;            /* device, any alignment: one block transfer's packet stream */
	uint64_t    len;               /* its bytes */
	/* in: the write */
	int64_t     offset_in_block;   /* of the write's first byte */
	int64_t     seqno;             /* of the write's first packet */
	int32_t     finish;            /* != 0: the empty lastPacketInBlock packet ends the write */
	int32_t     reserved;
	void       *wire;              /* device, any alignment: where the write's stream goes */
	uint64_t    wire_cap;          /* bytes of room at wire */
	/* out */
	uint64_t    consumed;          /* the read's: bytes of complete, framing-clean packets */
	uint64_t    delivered;         /* the read's: payload bytes of the packets before the first one with an error */
	int64_t     src_offset_in_block; /* packet 0's header field of the input (0: no packet) */
	uint64_t    wire_len;          /* bytes of the write's stream; 0 when rc != 0 */
	uint64_t    npkts;             /* its packets; 0 when rc != 0 */
	int32_t     rc;                /* the read's rc, or HDFS_CRC32C_EINVAL where the stream does not fit wire_cap */
	int32_t     path;              /* HDFS_RELAY_BATCH_PATH_* */
} hdfs_relay_batch_entry;

/* Relays the n entries e[0..n).  For every entry, rc, consumed and delivered
 * are those of
 *   hdfs_crc32c_read_packets(stream, len, proto, chunk_size, ctype, 0,
 *       HDFS_CRC32C_READ_ALL, ...)
 * of that stream alone with room for the whole payload: exactly what
 * hdfs_read_batch_read_blocks reports with a large enough destination.  If rc
 * == 0, wire[0, wire_len) is byte for byte what
 *   hdfs_wire_fused_compose_packets(payload, delivered, offset_in_block, seqno,
 *       proto, ctype, finish, ...)
 * writes for the payload that read delivers, and wire_len and npkts are that
 * call's.  An empty payload with finish is one header-only packet; without
 * finish it is nothing.  If rc != 0 the read found an error: wire_len == npkts
 * == 0 and the bytes of [wire, wire + wire_cap) are unspecified.  If the read
 * is clean but the stream needs more than wire_cap, the entry's rc is
 * HDFS_CRC32C_EINVAL, the text names the entry ("entry <k>") and the other
 * entries are served.  The call returns the first negative entry rc, else the
 * first nonzero one, else 0.  proto, chunk_size and ctype hold for the whole
 * batch and for both sides; ctype is CRC32 or CRC32C.
 *
 * No byte outside [wire, wire + wire_cap) is ever written, bytes of a clean
 * entry's wire range past wire_len are untouched, and only [stream, stream +
 * len) is read.
 *
 * Every stream and wire range is device memory of the engine's device at any
 * byte alignment, inside one device allocation; an entry with len == 0 names no
 * stream range, one with wire_cap == 0 no wire range.  Each of these is
 * HDFS_CRC32C_EINVAL for the whole call, decided before any device work, with
 * nothing written to any wire range, every entry's out fields zero and the
 * text naming the offending entry's index ("entry <k>"): n == 0, e == NULL,
 * more than HDFS_RELAY_BATCH_MAX_ENTRIES entries, a host pointer, a range that
 * leaves its allocation, a wire range that overlaps any stream or another wire
 * range of the batch, chunk_size == 0, a proto or ctype that is none, a
 * negative offset_in_block or seqno.  Streams may overlap each other or be
 * identical.
 *
 * ORDERING.  The work (one table upload, a probe launch, the main launch, one
 * copy of the descriptors back) is enqueued on `stream`, a hipStream_t of the
 * engine's device; NULL is a stream of this library that waits for the NULL
 * stream (a blocking stream): bytes written by other non-blocking streams
 * must then be complete before the call.  With a stream of the caller's, the
 * streams' bytes must be ordered ahead of the call on that stream.  The call
 * returns after the stream has been synchronised: the wire ranges' bytes are
 * then visible to every later operation on the device.  Entries that take the
 * fallback are served after that synchronise, one by one: the read under
 * hdfs_crc32c_read_packets' own rules, the framing on the same stream, each
 * synchronised before the next.  Calls from several threads are serialised
 * inside the library by one mutex (the CRC tables, uploaded once per device and
 * kept; the device tables, their pinned staging areas and the fallback's
 * payload buffer, grown on demand and kept). */
int hdfs_relay_batch_relay(hdfs_relay_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    void *stream);

/* Host only: the stream of a write of `payload` bytes at offset_in_block
 * (aligned or not), hdfs_wire_fused_compose_packets' wire_len and packet count.
 * Sizes a wire range before the read has run: payload is at most the stream's
 * length. */
int hdfs_relay_batch_layout(uint64_t payload, int64_t offset_in_block, int proto, int ctype, int finish,
    uint64_t *wire_len, uint64_t *npkts);

/* Measurement (tools/relay_batch_bench.py): hdfs_relay_batch_relay once on the
 * library's stream, then the probe and the main launch alone iters more times
 * between two HIP events; *ms_per_iter is their distance over iters.  flags:
 * HDFS_RELAY_BATCH_TIME_GROUPS(n) launches n workgroups (1..1024) instead of
 * the product's grid (one per compute unit); any other flag bit, n above 1024,
 * iters < 1 or a NULL ms_per_iter is HDFS_CRC32C_EINVAL before any device is
 * touched, with nothing written.  The entries' outputs and the bytes written
 * are the same under every flag. */
#define HDFS_RELAY_BATCH_TIME_GROUPS(n) ((unsigned)(n) << 8)
int hdfs_relay_batch_time(hdfs_relay_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_RELAY_BATCH_H */
