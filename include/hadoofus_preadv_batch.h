/*
 * hadoofus_preadv_batch.h -- a batch of scatter reads in one call: the packet
 * streams of many client reads, all in device memory, verified and the bytes
 * of each read's window laid over a list of device fragments by one launch,
 * one pass over the packets the reads take and one synchronise
 * (libhadoofus_preadv_batch.so, a companion of libhadoofus_crc32c.so built from
 * hadoofus_amd/csrc/preadv_batch*).
 *
 * A scatter read is hdfs_datanode_readv(d, off, iov, iovcnt, verifycsum)
 * (include/lowlevel.h:670, src/datanode.c:842-866; the per-packet copy loop is
 * _recv_packet_copy_data, src/datanode.c:2497-2537): a positional read whose
 * bytes go, in order, to the buffers of an iovec array -- the rows of a
 * tensor, the pages of a cache, a structure of arrays.  The main library takes
 * several device buffers in hdfs_crc32c_read_packets, one stream per call, and
 * with more than one buffer it verifies first and lays the bytes over the
 * buffers with a second launch.  libhadoofus_pread_batch.so batches positional
 * reads, each into ONE contiguous buffer.  This library is
 * hdfs_pread_batch_read with each entry's destination given as a list of device
 * fragments.
 *
 * Its kernel, unframe_scatter_batch_kernel, is the pread batch's with a scatter
 * store.  A probe launch frames packet 0 and the tail of every stream, works
 * out the window and cuts the entry to the packets the read takes; the main
 * launch loads and verifies every taken packet WHOLE and stores only the
 * window's bytes, destination position y (0 <= y < read_len) into the fragment
 * that holds byte y of the fragments' concatenation.  A 4 KiB round of a packet
 * that lies inside one fragment is stored as the pread batch stores it; a
 * round with fragment boundaries inside is stored piece by piece, 16 bytes at
 * a time where a lane's 16 bytes lie inside the piece and byte by byte at its
 * ends.  An entry whose stream or window is not of the shape the kernel takes,
 * or in which the main launch met a header or a CRC that is not the expected
 * one, is handed inside the call to hdfs_crc32c_read_packets with its window
 * and its own fragment list (path = HDFS_PREADV_BATCH_PATH_FALLBACK).  No
 * entry's result depends on which path it took.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  Against a loop of hdfs_crc32c_read_packets with the same
 * fragment lists: at every shape measured.  Against hdfs_pread_batch_read into
 * a contiguous buffer (a floor: the caller's scatter is still to be done, and
 * is not timed): level with it for one fragment a read, not clear of it for a
 * few large fragments, and well above it for many small ones, where the host's
 * work per fragment and the byte stores of seamed rounds decide.  One MI355X
 * (python tools/preadv_batch_bench.py; medians of 5
 * (min-max) per read with the paths alternated in one process after a warm-up
 * of each, host clock around each whole path, which ends in its synchronise,
 * CRC32C, v2, every read with a stream of its own of 64 KiB packets with the
 * empty last packet at odd addresses, its fragments of equal length 16 bytes
 * apart in rising address order, records kept, outputs and bytes of the paths
 * compared), microseconds per read:
 *   reads x window, c_begin, packets skipped, fragments   this call            loop of read_packets   pread batch, contiguous  launches alone
 *    256 x     65536 B   100  0      1 x      65 536 B  0.37 (0.36-0.50)     68.7 (68.0-69.0)       0.37 (0.36-0.43)     0.23
 *    256 x     65536 B   100  0     16 x       4 096 B  0.45 (0.44-0.51)     75.0 (74.9-75.3)       0.37 (0.36-0.41)     0.25
 *    256 x     65536 B   100  0  1 024 x          64 B  5.60 (5.52-9.53)     169.9 (169.7-171.6)    0.43 (0.40-0.44)     1.56
 *   1024 x      4096 B   100  0      1 x       4 096 B  0.18 (0.18-0.21)     18.8 (17.8-19.3)       0.20 (0.19-0.21)     0.12
 *   1024 x      4096 B   100  0     16 x         256 B  0.30 (0.29-0.30)     28.7 (28.7-28.9)       0.19 (0.18-0.20)     0.18
 *   1024 x      4096 B   100  0  1 024 x           4 B  7.54 (7.42-12.29)    125.8 (125.6-126.9)    0.23 (0.22-0.23)     2.79
 *     64 x   1048576 B   300  0      1 x   1 048 576 B  1.46 (1.43-1.72)     61.0 (60.5-61.4)       1.50 (1.49-1.70)     0.97
 *     64 x   1048576 B   300  0     16 x      65 536 B  1.61 (1.58-1.80)     67.6 (67.4-68.1)       1.46 (1.44-1.62)     1.07
 *     64 x   1048576 B   300  0  1 024 x       1 024 B  6.35 (5.98-6.37)     159.7 (159.6-160.7)    1.59 (1.56-1.61)     1.86
 *     16 x 134216728 B   500  0      1 x 134 216 728 B  65.3 (63.7-69.6)     84.5 (82.6-88.0)       65.4 (64.9-67.7)     58.97
 *     16 x 134216728 B   500  0     16 x   8 388 545 B  71.8 (70.1-77.8)     139.7 (136.4-146.3)    67.4 (66.3-69.3)     66.04
 *     16 x 134216728 B   500  0  1 024 x     131 071 B  83.0 (81.9-88.8)     202.4 (202.2-209.6)    67.7 (67.2-68.0)     71.69
 *    256 x     65536 B 30000 12      1 x      65 536 B  0.37 (0.36-0.53)     24.6 (24.4-24.8)       0.38 (0.38-0.45)     0.22
 *    256 x     65536 B 30000 12     16 x       4 096 B  0.50 (0.44-0.54)     36.9 (36.8-37.1)       0.41 (0.40-0.44)     0.23
 *    256 x     65536 B 30000 12  1 024 x          64 B  4.84 (4.56-5.10)     142.8 (142.7-143.2)    0.45 (0.44-0.47)     0.45
 *   1024 x      4096 B   100  0     64 x          64 B  0.75 (0.72-0.81)     42.0 (42.0-42.4)       0.22 (0.21-0.23)     0.37
 * (the last row: 4 KiB reads in 64-B fragments).  This call's range is clear of
 * the loop's in all sixteen rows: 1.3 to 2.4 times for 128 MiB reads, 17 to
 * 190 times for the others.  Against the pread batch: with ONE fragment a read
 * the ranges OVERLAP in all five rows (the unseamed round is that library's
 * store); with 16 fragments they overlap in two rows (1 MiB reads, and 64 KiB
 * reads from the middle of a stream) and this call is SLOWER in three (1.2
 * times for 64 KiB reads in 4 KiB fragments, 1.6 times for 4 KiB reads in
 * 256-B fragments, 1.07 times for 128 MiB reads in fragments of an odd length);
 * with 1 024 fragments it is slower in all five, 1.2 times for 128 MiB reads in
 * 128 KiB fragments, 4 times for 1 MiB reads in 1 KiB fragments, 11 to 33 times
 * for 64-B and 4-B fragments; 4 KiB reads in 64-B fragments cost 3.4 times the
 * contiguous read.  What a caller's own scatter of the staged bytes would add
 * to the pread batch's column was not measured, so these rows do not say which
 * of the two ways ends sooner.  Of the 5.6 microseconds of a 64 KiB read in
 * 1 024 fragments the launches are 1.6: the rest is the host's (the checks of
 * 262 144 fragments, their sweep, the table and its upload of 4 MiB).
 * Fragments in no address order cost the host a sort as well (an earlier run
 * that sorted always: 52 instead of 5.6 microseconds in that row).  Not
 * measured: CRC32, v1, a caller's stream, fallbacks in the batch, fragments in
 * shuffled address order, fragment lists that differ between the reads of a
 * batch, the caller's scatter after a contiguous read, a second run of the
 * command.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_preadv_batch_last_error()).
 */
#ifndef HADOOFUS_PREADV_BATCH_H
#define HADOOFUS_PREADV_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_PREADV_BATCH_<n>
 * (hadoofus_amd/csrc/preadv_batch_exports.map); run-time bindings compare
 * hdfs_preadv_batch_abi_version() with the version they were written for.  The
 * main library's ABI version and the other companions' are not affected. */
#define HDFS_PREADV_BATCH_ABI_VERSION 1

/* Most entries in one call. */
#define HDFS_PREADV_BATCH_MAX_ENTRIES 1024
/* Most non-empty fragments in one call, all entries together (the gather
 * batch's limit, HDFS_WIREV_FUSED_BATCH_MAX_FRAGS). */
#define HDFS_PREADV_BATCH_MAX_FRAGS (1u << 22)

#define HDFS_PREADV_BATCH_PATH_KERNEL   0   /* verified and delivered by this library's launch */
#define HDFS_PREADV_BATCH_PATH_FALLBACK 1   /* handed to hdfs_crc32c_read_packets inside the call */

int hdfs_preadv_batch_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_preadv_batch_last_error(void);

/* One scatter read of a batch, and what the call reports back about it. */
typedef struct hdfs_preadv_batch_entry {
	const void *stream;        /* in: the read's packet stream, device memory, any alignment */
	uint64_t    len;           /* in: its bytes */
	const hdfs_crc32c_iovec *iov; /* in: HOST array of the read's device fragments, any alignment each */
	int32_t     iovcnt;        /* in: its elements, >= 1 */
	int32_t     reserved;      /* in: 0 */
	int64_t     client_offset; /* in: the read's first byte in the block */
	int64_t     read_len;      /* in: the read's bytes, > 0 */
	/* out */
	uint64_t    consumed;      /* where the stream stands after the read (hdfs_crc32c_read_packets' *consumed) */
	uint64_t    delivered;     /* bytes laid over the fragments */
	uint64_t    npkts;         /* records at pkts + index * max_pkts */
	int32_t     rc;            /* this entry's hdfs_crc32c_read_packets result */
	int32_t     path;          /* HDFS_PREADV_BATCH_PATH_* */
} hdfs_preadv_batch_entry;

/* Serves the n scatter reads e[0..n).  For every entry b the outputs rc,
 * consumed, delivered, npkts, the records at pkts + b * max_pkts and the bytes
 * laid over the fragments in order are exactly what
 *   hdfs_crc32c_read_packets(stream, len, proto, chunk_size, ctype,
 *       client_offset, read_len, iov, iovcnt, pkts + b * max_pkts, max_pkts,
 *       &npkts, &consumed, &delivered)
 * of that entry alone returns and writes.  With cap the sum of the entry's
 * fragment lengths: HDFS_CRC32C_AGAIN with its resume point for cap <
 * read_len (continue with stream + consumed, client_offset + delivered,
 * read_len - delivered and further fragments),
 * HDFS_CRC32C_ERR_DATANODE_BAD_CHECKSUM with first_bad and bad_chunks,
 * HDFS_CRC32C_ERR_DATANODE_UNEXPECTED_READ_OFFSET,
 * HDFS_CRC32C_ERR_DATANODE_BAD_LASTPACKET, every framing error, a walk that
 * ends at an incomplete packet, a run cut by max_pkts, chunk_size != 512, and
 * that call's EINVAL for a negative client_offset (rc is then negative and the
 * text names the entry; the other entries are served).  These entries are
 * handed to that function inside the call (path FALLBACK).  Empty fragments
 * are skipped, and one may have a NULL base, as in the main call.  An entry
 * with len == 0 or cap == 0 names no range and goes to the fallback.  The
 * layout of the records is hdfs_pread_batch_read's: one max_pkts for all
 * entries, entry b's records at pkts + b * max_pkts.  pkts == NULL: no records
 * are wanted, max_pkts is not looked at and no walk is cut; everything else is
 * unchanged.  The call returns the first negative entry rc, else the first
 * nonzero one, else 0.  proto, chunk_size and ctype hold for the whole batch;
 * ctype is CRC32 or CRC32C (HDFS_CRC32C_CSUM_NULL is EINVAL, as in the main
 * call).
 *
 * Fragment bytes past delivered are unspecified, up to destination position
 * min(cap, read_len).  Nothing past that position is written, whole trailing
 * fragments included, and only [stream, stream + len) is read.
 *
 * Every stream and every non-empty fragment is device memory of the engine's
 * device at any byte alignment, inside one device allocation.  Each of these
 * is HDFS_CRC32C_EINVAL for the whole call, decided before any device work,
 * with nothing written to any fragment or record, every entry's rc, consumed,
 * delivered and npkts zero (its path is HDFS_PREADV_BATCH_PATH_FALLBACK: no
 * launch of this library served it) and the text naming the offending entry's
 * index and, where there is one, the fragment's ("entry <k>", "fragment <i>"):
 * n == 0, e == NULL, more than HDFS_PREADV_BATCH_MAX_ENTRIES entries,
 * read_len <= 0 (whole payloads, HDFS_CRC32C_READ_ALL, are
 * hdfs_read_batch_read_blocks' job, and the text says so), chunk_size == 0, a
 * proto or ctype that is none, a NULL stream with a length, iovcnt < 1 or a
 * NULL iov, a NULL base with a length, more than HDFS_PREADV_BATCH_MAX_FRAGS
 * non-empty fragments in the call (these counts and limits are checked before
 * any pointer is looked at), a host pointer, a range that leaves its
 * allocation, a non-empty fragment that overlaps any stream of the batch or
 * another fragment of the batch, the same entry's included.  Streams may
 * overlap each other or be identical: many reads of one stream are many
 * entries.
 *
 * ORDERING.  The work (one table upload, a probe launch, the main launch, one
 * copy of the descriptors back) is enqueued on `stream`, a hipStream_t of the
 * engine's device; NULL is a stream of this library that waits for the NULL
 * stream (a blocking stream): bytes written by other non-blocking streams
 * must then be complete before the call.  With a stream of the caller's, the
 * streams' bytes must be ordered ahead of the call on that stream.  The call
 * returns after the stream has been synchronised: the fragments' bytes are
 * then visible to every later operation on the device.  Entries handed to
 * hdfs_crc32c_read_packets are read after that synchronise, one by one, under
 * that call's own rules.  Calls from several threads are serialised inside the
 * library by one mutex (the CRC tables, uploaded once per device and kept; one
 * device table and one pinned staging area, grown on demand and kept). */
int hdfs_preadv_batch_read(hdfs_preadv_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    hdfs_crc32c_packet *pkts, size_t max_pkts, void *stream);

/* Measurement (tools/preadv_batch_bench.py): hdfs_preadv_batch_read once on the
 * library's stream without records, then the probe and the main launch alone
 * iters more times between two HIP events; *ms_per_iter is their distance
 * over iters.  flags: HDFS_PREADV_BATCH_TIME_GROUPS(n) launches n workgroups
 * (1..1024) instead of the product's grid (one per compute unit), so that
 * every workgroup walks many packets across the entries; any other flag bit, n
 * above 1024, iters < 1 or a NULL ms_per_iter is HDFS_CRC32C_EINVAL before any
 * device is touched, with nothing written.  The entries' outputs and the bytes
 * delivered are the same under every flag. */
#define HDFS_PREADV_BATCH_TIME_GROUPS(n) ((unsigned)(n) << 8)
int hdfs_preadv_batch_time(hdfs_preadv_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_PREADV_BATCH_H */
