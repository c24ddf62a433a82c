/*
 * hadoofus_pread_batch.h -- a batch of positional reads in one call: the
 * packet streams of many client reads, all in device memory, verified and the
 * bytes of each read's window delivered into device buffers by one launch, one
 * pass over the packets the reads take and one synchronise
 * (libhadoofus_pread_batch.so, a companion of libhadoofus_crc32c.so built from
 * hadoofus_amd/csrc/pread_batch*).
 *
 * A positional read is hdfs_datanode_read(bloff, len) (src/datanode.c:1363-1377,
 * the read loop at :1476-1481, the window arithmetic at :2478-2549): the
 * datanode's stream starts at a chunk boundary at or before the wanted offset,
 * so packet 0 carries up to 511 bytes (or more, with a stream cut from a longer
 * one) the caller did not ask for, and the read may stop short of the stream's
 * end.  The main library serves it one stream per call,
 * hdfs_crc32c_read_packets with read_len > 0, and every call pays a launch's
 * fixed cost, the framing and a synchronise.  libhadoofus_read_batch.so
 * batches whole-block reads only (client_offset 0, HDFS_CRC32C_READ_ALL).
 * This library runs the windowed call for N reads at once.
 *
 * Its kernel, unframe_window_batch_kernel, is the read batch's with a windowed
 * store.  A probe launch frames packet 0 and the tail of every stream, works
 * out the window (c_begin, the m packets up to the one that completes the
 * read) and cuts the entry to those m packets: later packets, the empty last
 * one included, are neither read nor returned, so a 64 KiB window in a 128 MiB
 * stream costs one or two packets.  The main launch loads and verifies every
 * taken packet WHOLE -- a corrupt chunk in the skipped head of packet 0, or
 * behind the read's end in the last taken packet, is BAD_CHECKSUM, as in the
 * reference, which verifies a packet before it copies any of it -- and stores
 * only the window's bytes.  An entry whose stream or window is not of the
 * shape the kernel takes, or in which the main launch met a header or a CRC
 * that is not the expected one, is handed inside the call to
 * hdfs_crc32c_read_packets with its window (path =
 * HDFS_PREAD_BATCH_PATH_FALLBACK).  No entry's result depends on which path it
 * took.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  Against a loop of windowed hdfs_crc32c_read_packets over the
 * same entries: at every shape measured.  Against hdfs_read_batch_read_blocks
 * of the same streams (whole payloads, the window still to be copied out):
 * where the reads are many and small or end early; not for large windows that
 * cover nearly the whole stream.  One MI355X (python
 * tools/pread_batch_bench.py; medians of 5 (min-max) per
 * read with the paths alternated in one process after a warm-up of each, host
 * clock around each whole path, which ends in its synchronise, CRC32C, v2,
 * every read with a stream of its own of 64 KiB packets with the empty last
 * packet at odd addresses, records kept, outputs and delivered bytes of the
 * paths compared), microseconds per read:
 *     reads x window, stream, c_begin              this call          loop of read_packets  READ_ALL batch      launches alone
 *      256 x 64 KiB, 64.5 KiB stream, 100          0.39 (0.37-0.49)   70.0 (69.2-70.1)      0.49 (0.49-0.53)    0.23
 *     1024 x  4 KiB, 4.5 KiB stream, 100           0.20 (0.19-0.22)   19.0 (18.8-19.2)      0.79 (0.78-0.80)    0.13
 *       64 x  1 MiB, 1 MiB + 512 B stream, 300     1.50 (1.49-1.73)   63.3 (63.1-63.6)      1.45 (1.45-1.58)    1.00
 *       16 x 128 MiB - 1000 B, 128 MiB, 500        68.9 (68.1-73.1)   86.0 (85.1-91.6)      73.1 (72.0-75.8)    63.4
 *      256 x 64 KiB, from packet 12 on of a
 *            2 MiB stream (its middle), 30000      0.39 (0.39-0.46)   27.2 (27.1-27.3)      1.15 (1.13-1.25)    0.23
 * This call's range is clear of the loop's in all five rows (1.2 times for
 * 128 MiB reads, 42 to 178 times for small ones).  Against the read batch's
 * READ_ALL call: 4 times faster for 1 024 reads of 4 KiB (in that run that call
 * compared every pair of entries for overlaps and this one sorted them; since
 * then both call the one sweep of companion_support.h, see below) and 2.9 times where
 * the stream is taken from the middle of a longer one and the read ends early
 * (the last row: 2 packets taken of 21, READ_ALL walks and delivers the whole
 * stream); the ranges OVERLAP in the other three rows, and at 1 MiB this
 * call's median is the higher one: for a window that is nearly the whole
 * stream it saves nothing over READ_ALL.  A workgroup takes one packet a
 * step, so streams of tiny packets cost a step each.  Not measured: CRC32, v1,
 * a caller's stream, fallbacks in the batch, many reads of one shared stream, a
 * second run of the command.
 * Since the read batch calls the shared sweep too, a later run of the same
 * command (--quick) gave for 1 024 x 4 KiB: this call 0.188 (0.185-0.202), the
 * READ_ALL batch 0.214 (0.208-0.232), 1.1 times apart.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_pread_batch_last_error()).
 */
#ifndef HADOOFUS_PREAD_BATCH_H
#define HADOOFUS_PREAD_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_PREAD_BATCH_<n>
 * (hadoofus_amd/csrc/pread_batch_exports.map); run-time bindings compare
 * hdfs_pread_batch_abi_version() with the version they were written for.  The
 * main library's ABI version and the other companions' are not affected. */
#define HDFS_PREAD_BATCH_ABI_VERSION 1

/* Most entries in one call. */
#define HDFS_PREAD_BATCH_MAX_ENTRIES 1024

#define HDFS_PREAD_BATCH_PATH_KERNEL   0   /* verified and delivered by this library's launch */
#define HDFS_PREAD_BATCH_PATH_FALLBACK 1   /* handed to hdfs_crc32c_read_packets inside the call */

int hdfs_pread_batch_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_pread_batch_last_error(void);

/* One positional read of a batch, and what the call reports back about it. */
typedef struct hdfs_pread_batch_entry {
	const void *stream;        /* in: the read's packet stream, device memory, any alignment */
	uint64_t    len;           /* in: its bytes */
	void       *dst;           /* in: device destination of the read's bytes, any alignment */
	uint64_t    dst_cap;       /* in: bytes of room at dst */
	int64_t     client_offset; /* in: the read's first byte in the block */
	int64_t     read_len;      /* in: the read's bytes, > 0 */
	/* out */
	uint64_t    consumed;      /* where the stream stands after the read (hdfs_crc32c_read_packets' *consumed) */
	uint64_t    delivered;     /* bytes at dst */
	uint64_t    npkts;         /* records at pkts + index * max_pkts */
	int32_t     rc;            /* this entry's hdfs_crc32c_read_packets result */
	int32_t     path;          /* HDFS_PREAD_BATCH_PATH_* */
} hdfs_pread_batch_entry;

/* Serves the n positional reads e[0..n).  For every entry b the outputs rc,
 * consumed, delivered, npkts, the records at pkts + b * max_pkts and the bytes
 * dst[0, delivered) are exactly what
 *   hdfs_crc32c_read_packets(stream, len, proto, chunk_size, ctype,
 *       client_offset, read_len, &{dst, dst_cap}, 1, pkts + b * max_pkts,
 *       max_pkts, &npkts, &consumed, &delivered)
 * returns and writes: HDFS_CRC32C_AGAIN with its resume point for a
 * destination smaller than the read (continue with stream + consumed,
 * client_offset + delivered, read_len - delivered and a further buffer),
 * HDFS_CRC32C_ERR_DATANODE_BAD_CHECKSUM with first_bad and bad_chunks,
 * HDFS_CRC32C_ERR_DATANODE_UNEXPECTED_READ_OFFSET,
 * HDFS_CRC32C_ERR_DATANODE_BAD_LASTPACKET, every framing error, a walk that
 * ends at an incomplete packet, a run cut by max_pkts, and that call's EINVAL
 * for a negative client_offset (rc is then negative and the text names the
 * entry; the other entries are served).  The layout of the records is
 * hdfs_read_batch_read_blocks': one max_pkts for all entries, entry b's
 * records at pkts + b * max_pkts.  pkts == NULL: no records are wanted,
 * max_pkts is not looked at and no walk is cut; everything else is unchanged.
 * The call returns the first negative entry rc, else the first nonzero one,
 * else 0.  proto, chunk_size and ctype hold for the whole batch; ctype is
 * CRC32 or CRC32C (HDFS_CRC32C_CSUM_NULL is EINVAL, as in the main call).
 *
 * Bytes of dst past delivered are unspecified.  No byte outside [dst, dst +
 * min(dst_cap, read_len)) is written, and only [stream, stream + len) is read.
 *
 * Every stream and destination range is device memory of the engine's device
 * at any byte alignment, inside one device allocation; an entry with len == 0
 * or dst_cap == 0 names no such range.  Each of these is HDFS_CRC32C_EINVAL
 * for the whole call, decided before any device work, with nothing written to
 * any destination or record, every entry's rc, consumed, delivered and npkts
 * zero (its path is HDFS_PREAD_BATCH_PATH_FALLBACK: no launch of this library
 * served it) and the text naming the offending entry's index ("entry <k>"):
 * n == 0, e == NULL, more than
 * HDFS_PREAD_BATCH_MAX_ENTRIES entries, read_len <= 0 (whole payloads,
 * HDFS_CRC32C_READ_ALL, are hdfs_read_batch_read_blocks' job, and the text
 * says so), a host pointer, a range that leaves its allocation, a destination
 * that overlaps any stream or another destination of the batch over [dst, dst
 * + dst_cap), chunk_size == 0, a proto or ctype that is none.  Streams may
 * overlap each other or be identical: many reads of one stream are many
 * entries.
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
int hdfs_pread_batch_read(hdfs_pread_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    hdfs_crc32c_packet *pkts, size_t max_pkts, void *stream);

/* Measurement (tools/pread_batch_bench.py): hdfs_pread_batch_read once on the
 * library's stream without records, then the probe and the main launch alone
 * iters more times between two HIP events; *ms_per_iter is their distance
 * over iters.  flags: HDFS_PREAD_BATCH_TIME_GROUPS(n) launches n workgroups
 * (1..1024) instead of the product's grid (one per compute unit), so that
 * every workgroup walks many packets across the entries; any other flag bit, n
 * above 1024, iters < 1 or a NULL ms_per_iter is HDFS_CRC32C_EINVAL before any
 * device is touched, with nothing written.  The entries' outputs and the bytes
 * delivered are the same under every flag. */
#define HDFS_PREAD_BATCH_TIME_GROUPS(n) ((unsigned)(n) << 8)
int hdfs_pread_batch_time(hdfs_pread_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_PREAD_BATCH_H */
