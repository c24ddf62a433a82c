/*
 * hadoofus_read_batch.h -- a batch of block reads in one call: the packet
 * streams of many block transfers, all in device memory, verified and
 * de-framed into device buffers by one launch, one pass over the bytes and one
 * synchronise (libhadoofus_read_batch.so, a companion of libhadoofus_crc32c.so
 * built from hadoofus_amd/csrc/read_batch*).
 *
 * The main library delivers data one stream at a time:
 * hdfs_crc32c_read_packets verifies one packet stream and de-frames it, and
 * every call pays a launch's fixed cost, the framing and a synchronise;
 * hdfs_crc32c_verify_blocks_submit takes 16 blocks a launch but delivers no
 * byte.  A client that reads a file of many blocks into GPU memory -- the
 * per-block read loop of src/datanode.c:1476-1482, run once per block --
 * loops over hdfs_crc32c_read_packets.  This library runs that loop for N
 * blocks in one call.  It is the read-side twin of
 * hdfs_wire_fused_batch_compose (hadoofus_wire_fused_batch.h) and its kernel,
 * unframe_fused_batch_kernel, runs that library's round the other way: the
 * packet's data region is loaded, the same registers are stored to the
 * destination, and the chunk CRCs computed from them are compared with the
 * packet's CRC bytes instead of stored.
 *
 * A datanode's stream is predictable from its first packet (K packets of one
 * size, at most one shorter one, at most one empty last one), so a probe
 * launch frames only packet 0 and the tail of every stream, and the main
 * launch compares every header it meets with the one the prediction composes.
 * An entry whose stream is not of that shape, or in which the main launch met
 * a header or a CRC that is not the expected one, is handed inside the call to
 * hdfs_crc32c_read_packets, which yields the exact records and overwrites the
 * destination (path = HDFS_READ_BATCH_PATH_FALLBACK).  No entry's result
 * depends on which path it took.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  At every shape measured, against a loop of
 * hdfs_crc32c_read_packets over the same entries.  One MI355X
 * (tools/read_batch_bench.py; medians of 5 (min-max) per
 * block with the paths alternated in one process after a warm-up of each, host
 * clock around each whole path, which ends in its synchronise, CRC32C, v2,
 * streams with the empty last packet at odd addresses, records kept, outputs
 * and delivered bytes of both paths compared), microseconds per block:
 *     blocks x size              this call           loop of read_packets   launches alone
 *       16 x 128 MiB             74.2 (73.3-80.8)    83.8 (82.2-91.0)       68.2
 *       64 x 128 MiB             72.6 (71.8-79.0)    82.7 (82.5-86.2)       67.7
 *       15 x 128 MiB + 5 MiB     69.0 (68.4-72.9)    79.1 (78.4-84.3)       64.3
 *       64 x 128 MiB, 1 corrupt  74.2 (73.1-81.3)    83.2 (82.7-86.6)       67.7
 *       64 x   1 MiB             1.33 (1.30-1.95)    25.1 (25.1-25.8)       0.93
 *      256 x  64 KiB             0.82 (0.60-1.02)    23.6 (23.2-23.8)       0.21
 * This call's range is clear of the loop's in all six rows: 1.12 to 1.15 times
 * for 128 MiB blocks (the per-block launch, framing and synchronise are what is
 * saved), 19 and 29 times for small blocks, where the loop pays 23 to 25 us per
 * call whatever the size.  One corrupted block of 64 (the fifth row) costs the
 * call one hdfs_crc32c_read_packets of that block, about 0.1 ms.  Where it is
 * weak: a workgroup takes one packet a step, as in the fused batch write
 * library, so streams of tiny packets cost a step each; and verification
 * alone, which delivers no byte (hdfs_crc32c_verify_blocks_submit in jobs of
 * 16: 23 to 29 us per 128 MiB block), stays 2.5 to 3 times faster.  Not
 * measured: CRC32, v1, a caller's stream, many fallbacks in one batch, a second
 * run of the command.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_read_batch_last_error()).
 */
#ifndef HADOOFUS_READ_BATCH_H
#define HADOOFUS_READ_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_READ_BATCH_<n>
 * (hadoofus_amd/csrc/read_batch_exports.map); run-time bindings compare
 * hdfs_read_batch_abi_version() with the version they were written for.  The
 * main library's ABI version and the other companions' are not affected. */
#define HDFS_READ_BATCH_ABI_VERSION 1

/* Most entries in one call. */
#define HDFS_READ_BATCH_MAX_ENTRIES 1024

#define HDFS_READ_BATCH_PATH_KERNEL   0   /* verified and delivered by this library's launch */
#define HDFS_READ_BATCH_PATH_FALLBACK 1   /* handed to hdfs_crc32c_read_packets inside the call */

int hdfs_read_batch_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_read_batch_last_error(void);

/* One block transfer of a batch, and what the call reports back about it. */
typedef struct hdfs_read_batch_entry {
	const void *stream;       /* in: one block transfer's packet stream, device memory, any alignment */
	uint64_t    len;          /* in: its bytes */
	void       *dst;          /* in: device destination of its payload, any alignment */
	uint64_t    dst_cap;      /* in: bytes of room at dst */
	/* out */
	uint64_t    consumed;     /* bytes of complete, framing-clean packets */
	uint64_t    delivered;    /* payload bytes of the packets before the first one with an error */
	uint64_t    npkts;        /* records at pkts + index * max_pkts */
	int32_t     rc;           /* this entry's hdfs_crc32c_read_packets result */
	int32_t     path;         /* HDFS_READ_BATCH_PATH_* */
} hdfs_read_batch_entry;

/* Reads the n block transfers e[0..n).  For every entry b the outputs rc,
 * consumed, delivered, npkts, the records at pkts + b * max_pkts and the bytes
 * dst[0, delivered) are exactly what
 *   hdfs_crc32c_read_packets(stream, len, proto, chunk_size, ctype, 0,
 *       HDFS_CRC32C_READ_ALL, &{dst, dst_cap}, 1, pkts + b * max_pkts,
 *       max_pkts, &npkts, &consumed, &delivered)
 * returns and writes: every framing error, HDFS_CRC32C_ERR_DATANODE_BAD_CHECKSUM
 * with first_bad and bad_chunks, the empty last packet, an incomplete last
 * packet (the walk ends ahead of it), a run cut by max_pkts, and that call's
 * EINVAL for a destination smaller than the framed payload (rc is then
 * negative and the text names the entry; the other entries are served).  The
 * layout of the records is hdfs_crc32c_job_wait_blocks': one max_pkts for all
 * entries, entry b's records at pkts + b * max_pkts.  pkts == NULL: no records
 * are wanted, max_pkts is not looked at and no walk is cut; everything else
 * is unchanged.  The call returns the first negative entry rc, else the first
 * nonzero one, else 0.  proto, chunk_size and ctype hold for the whole batch;
 * ctype is CRC32 or CRC32C (HDFS_CRC32C_CSUM_NULL is EINVAL, as in the main
 * call).
 *
 * Bytes of dst past delivered are unspecified.  No byte outside [dst, dst +
 * dst_cap) is written, and only [stream, stream + len) is read.
 *
 * Every stream and destination range is device memory of the engine's device
 * at any byte alignment, inside one device allocation; an entry with len == 0
 * or dst_cap == 0 names no such range.  Each of these is HDFS_CRC32C_EINVAL
 * for the whole call, decided before any device work, with nothing written to
 * any destination or record, every entry's out fields zero and the text naming
 * the offending entry's index ("entry <k>"): n == 0, e == NULL, more than
 * HDFS_READ_BATCH_MAX_ENTRIES entries, a host pointer, a range that leaves
 * its allocation, a destination that overlaps any stream or another
 * destination of the batch, chunk_size == 0, a proto or ctype that is none.
 * Streams may overlap each other or be identical.
 *
 * ORDERING.  The work (one table upload, a probe launch, the main launch, one
 * copy of the descriptors back) is enqueued on `stream`, a hipStream_t of the
 * engine's device; NULL is a stream of this library that waits for the NULL
 * stream (a blocking stream): bytes written by other non-blocking streams
 * must then be complete before the call.  With a stream of the caller's, the
 * streams' bytes must be ordered ahead of the call on that stream.  The call
 * returns after the stream has been synchronised: the destinations' bytes are
 * then visible to every later operation on the device.  Entries handed to
 * hdfs_crc32c_read_packets are read after that synchronise, one by one, under
 * that call's own rules.  Calls from several threads are serialised inside the
 * library by one mutex (the CRC tables, uploaded once per device and kept; one
 * device table and one pinned staging area, grown on demand and kept). */
int hdfs_read_batch_read_blocks(hdfs_read_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    hdfs_crc32c_packet *pkts, size_t max_pkts, void *stream);

/* Measurement (tools/read_batch_bench.py): hdfs_read_batch_read_blocks once on
 * the library's stream without records, then the probe and the main launch
 * alone iters more times between two HIP events; *ms_per_iter is their
 * distance over iters.  flags: HDFS_READ_BATCH_TIME_GROUPS(n) launches n
 * workgroups (1..1024) instead of the product's grid (one per compute unit),
 * so that every workgroup walks many packets across the entries; any other
 * flag bit, n above 1024, iters < 1 or a NULL ms_per_iter is
 * HDFS_CRC32C_EINVAL before any device is touched, with nothing written.  The
 * entries' outputs and the bytes delivered are the same under every flag. */
#define HDFS_READ_BATCH_TIME_GROUPS(n) ((unsigned)(n) << 8)
int hdfs_read_batch_time(hdfs_read_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_READ_BATCH_H */
