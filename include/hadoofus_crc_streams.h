/*
 * hadoofus_crc_streams.h -- composite CRCs (HDFS's COMPOSITE_CRC checksum
 * mode) of blocks and files taken from packet streams in device memory
 * (libhadoofus_crc_streams.so, a companion of libhadoofus_crc32c.so built from
 * hadoofus_amd/csrc/crc_streams*).
 *
 * The main library combines chunk CRCs that a compute plan left in a device
 * array (hdfs_crc32c_composite_crcs).  The fused write libraries
 * (hdfs_wire_fused_batch_compose and its kin) and the read batch libraries
 * (hdfs_read_batch_read_blocks and its kin) have no compute plan and no CRC
 * array: their chunk CRCs exist only inside the wire streams, between the
 * packets' headers and data.  This library combines them where they lie.  The
 * combine is associative, c(A || B) = c(A) * x^(8 |B|) ^ c(B) mod P, so every
 * packet's CRCs are folded by a wave of their own and the packets of a block
 * by the lanes of one wave; there is no chain as in MD5CRC
 * (hadoofus_md5crc_streams.h).  Of a stream it reads the headers and the CRC
 * bytes, 1/128 of it at 512 bytes per CRC.
 *
 * THE CRCS ARE NOT VERIFIED HERE.  No data byte is read, so a CRC that does
 * not belong to its chunk is combined as it stands.  Verification is the read
 * batch's (hdfs_read_batch_read_blocks compares every CRC with its chunk) or
 * not needed (the fused write computed the CRCs from the data it framed).
 * The value is the block's COMPOSITE_CRC when the stream carries the whole
 * block: offset_in_block == 0, nothing missing at the end (rc == 0 and
 * consumed == len, or a payload the caller knows).  The caller sees all of
 * that in the entry's out fields; hdfs_crc_streams_file_checksum insists on
 * offset_in_block == 0.  Unlike MD5CRC the value does not depend on the chunk
 * size or on how the payload is cut into packets and blocks.
 *
 * A datanode's stream is predictable from its first packet (K packets of one
 * size, at most one shorter one, at most one empty last one).  A probe launch
 * frames only packet 0 and the tail of every stream; a second launch compares
 * every packet's header with the one the prediction composes and folds the CRC
 * region behind it into the packet's CRC; a third reduces every entry's
 * packets, a wave an entry.  An entry whose stream is not of that shape, or
 * whose headers are not the predicted ones, or whose packets lie past the
 * 2^25 packets a call keeps a table for, is handed inside the call to
 * hdfs_crc32c_parse_packets, and the packets that walk records are folded and
 * reduced by the same two kernels (path = HDFS_CRC_STREAMS_PATH_FALLBACK).  No
 * entry's result depends on which path it took.  No CRC arithmetic of a
 * stream's chunks happens on the host.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  In time and in memory for a datanode's 64 KiB packets, at
 * every shape measured; not in time for small packets.  One MI355X
 * (tools/crc_streams_bench.py, DESIGN.md section 24,
 * profiles/crc_streams_bench.json; v2, CRC32C, every block its own payload and
 * its own stream at an odd address; medians of 5 (min-max) with the paths
 * alternated in one process after a warm-up of each, host clock around each
 * whole path, which ends in its synchronise; the CRCs of the first three paths
 * compared), milliseconds per call:
 *     blocks x size              this call          plan + composite_crcs   composite_crcs alone   md5crc streams        launches alone
 *        1 x 128 MiB             0.057 (0.056-0.076)  0.121 (0.121-0.142)    0.089 (0.089-0.092)    18.4 (17.7-20.0)      0.038
 *       64 x 128 MiB             0.260 (0.258-0.301)  1.50 (1.48-1.51)       0.187 (0.175-0.207)    28.8 (28.7-28.9)      0.233
 *      256 x 128 MiB             0.894 (0.884-0.916)  7.09 (7.00-7.20)       0.837 (0.826-0.857)    31.7 (31.6-31.7)      0.828
 *      896 x 128 MiB             3.02 (2.99-3.03)     22.4 (22.3-22.5)       2.45 (2.38-2.50)       32.1 (32.1-32.2)      2.79
 *      256 x 128 MiB, 5 KiB pkts 6.97 (6.97-6.99)     6.57 (6.44-6.68)       0.831 (0.827-0.842)    115.5 (115.1-116.1)   6.62
 *     1024 x   1 MiB             0.198 (0.193-0.211)  0.290 (0.288-0.308)    0.168 (0.168-0.170)    0.347 (0.337-0.351)   0.140
 * "plan + composite_crcs" is what a caller does without this library: a compute
 * plan over the payloads (created beforehand, executed in the measurement) and
 * hdfs_crc32c_composite_crcs over the CRC arrays it leaves; "composite_crcs
 * alone" the same combine over CRC arrays packed beforehand, a floor; "md5crc
 * streams" hdfs_md5crc_streams_block_digests of the same streams, HDFS's other
 * checksum mode.  896 blocks are what the device's memory held of payloads and
 * streams together.  Every path is timed as a C caller runs it: the raw
 * library call on arrays built beforehand.  Row by row: this call is FASTER
 * than the compute plan plus hdfs_crc32c_composite_crcs for 1, 64, 256 and 896
 * blocks of 128 MiB in 64 KiB packets (2.1, 5.8, 7.9 and 7.4 times) and for
 * 1 024 blocks of 1 MiB (1.5 times).  Against the floor it is below it for one
 * block only (0.057 against 0.089 ms) and ABOVE it everywhere else: 1.4, 1.1 and
 * 1.2 times for 64, 256 and 896 blocks, 1.2 times for 1 024 blocks of 1 MiB (the
 * header check and one wave a packet against a packed array).  It is SLOWER
 * than the plan, 1.06 times, for 256 blocks of 128 MiB in 5 120-byte packets,
 * and 8 times above the floor there: the time goes into the fold launch, which
 * spends a wave, a header comparison, a lookup and three multiplies on every
 * packet whatever its size -- 6.7 million packets of ten CRCs each, nine of 64
 * lanes busy -- about 1 ns a packet against 1.5 ns for a packet of 128 CRCs.
 * Against MD5CRC from the same streams it is 11 to 320 times faster for 128 MiB
 * blocks: no chain.  In
 * memory: no payload is needed and no CRC array, but a table of 4 B per packet,
 * which has to be sized before the probe has run -- 4 B for every 541 bytes of
 * stream, what the smallest regular packet takes, at most 128 MiB.  Up to 16
 * GiB of streams a call that is as much as the CRC array it replaces; above, it
 * stays 128 MiB (896 blocks: 128 MiB held, 7 MiB used, against 896 MiB of CRC
 * array).  Not measured: CRC32, v1, a
 * caller's stream, entries that fall back, chunk sizes other than 512, streams
 * of 512-byte packets, LDS byte tables in place of the multiplies, a second
 * run of the command.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_crc_streams_last_error()).
 */
#ifndef HADOOFUS_CRC_STREAMS_H
#define HADOOFUS_CRC_STREAMS_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_CRC_STREAMS_<n>
 * (hadoofus_amd/csrc/crc_streams_exports.map); run-time bindings compare
 * hdfs_crc_streams_abi_version() with the version they were written for.  The
 * main library's ABI version and the other companions' are not affected. */
#define HDFS_CRC_STREAMS_ABI_VERSION 1

/* Most entries in one call. */
#define HDFS_CRC_STREAMS_MAX_ENTRIES 1024

#define HDFS_CRC_STREAMS_PATH_KERNEL   0   /* framed by the probe, folded where the CRCs lie */
#define HDFS_CRC_STREAMS_PATH_FALLBACK 1   /* framed by hdfs_crc32c_parse_packets inside the call */

int hdfs_crc_streams_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_crc_streams_last_error(void);

/* One block's packet stream, and what the call reports back about it. */
typedef struct hdfs_crc_streams_entry {
	const void *stream;          /* in: packet stream, device memory, any byte alignment */
	uint64_t    len;             /* in: its bytes */
	/* out */
	uint64_t    consumed;        /* bytes of complete, framing-clean packets */
	uint64_t    payload;         /* their data bytes */
	uint64_t    nchunks;         /* CRCs combined */
	uint64_t    npkts;           /* packets walked */
	int64_t     offset_in_block; /* packet 0's header field (0 when there is no packet) */
	int32_t     rc;              /* this entry's hdfs_crc32c_parse_packets result */
	int32_t     path;            /* HDFS_CRC_STREAMS_PATH_* */
	uint32_t    crc;             /* composite CRC of the payload, host order */
	uint32_t    reserved;        /* 0 */
} hdfs_crc_streams_entry;

/* A file's COMPOSITE_CRC checksum.  The tag alone names it (struct
 * hdfs_crc_streams_file_checksum): the function below has the same name, and a
 * typedef would share C's ordinary name space with it. */
struct hdfs_crc_streams_file_checksum {
	uint32_t bytes_per_crc;      /* the call's chunk_size (the value does not depend on it) */
	uint32_t ctype;              /* HDFS_CRC32C_CSUM_CRC32 or _CRC32C */
	uint32_t crc;                /* the file's composite CRC, host order */
	uint8_t  bytes[4];           /* crc big-endian: the checksum's wire bytes */
	uint64_t length;             /* sum of the blocks' payload */
};

/* Combines the CRCs of the n streams e[0..n).  For every entry b: rc, consumed
 * and npkts are those of hdfs_crc32c_parse_packets(stream, len, proto,
 * chunk_size, ctype, ...) of that stream alone with unlimited record room;
 * payload is the sum of the framing-clean records' data_len and nchunks the
 * sum of their crc_len / 4.  When rc == 0, crc is the combine of the CRC words
 * of the recorded packets as they stand in the stream (big-endian there, host
 * order here), each over its chunk's length: a packet of d data bytes holds
 * ceil(d / chunk_size) CRCs, the last of them over d - chunk_size * (n - 1)
 * bytes, whichever packet of the stream it is.  When the CRCs are the chunks'
 * own, crc is the CRC (zlib's crc32, or CRC32C, from 0) of the delivered
 * payload bytes.  The empty last packet contributes nothing, an incomplete
 * last packet ends the walk ahead of it.  A stream without a complete packet,
 * len == 0 (stream may then be NULL) or only the empty last packet gives rc 0,
 * crc 0 and nchunks 0.  When rc != 0 (a framing error) crc and nchunks are 0;
 * consumed, npkts and payload stay the walk's.  The call returns the first
 * negative entry rc, else the first nonzero one, else 0.  proto, chunk_size and
 * ctype hold for the whole batch.  The entries handed to
 * hdfs_crc32c_parse_packets may have 2^29 - 1 packets with CRCs between them
 * in one call; the entry that goes past that gets rc HDFS_CRC32C_EINVAL, crc 0
 * and the text "entry <k>: too many packets", and being negative that is what
 * the call returns.
 *
 * Only [stream, stream + consumed) is read, and of it no data byte.  Nothing
 * is written to device memory the caller owns.
 *
 * Every stream is device memory of the engine's device at any byte alignment,
 * inside one device allocation; an entry with len == 0 names no range.  Each of
 * these is HDFS_CRC32C_EINVAL for the whole call, decided before any device
 * work, with every entry's out fields zero and the text naming the offending
 * entry's index ("entry <k>"; the batch's own arguments count as entry 0's):
 * n == 0, e == NULL, more than HDFS_CRC_STREAMS_MAX_ENTRIES entries, a host
 * pointer, a range that leaves its allocation, chunk_size == 0, a proto that is
 * none, a ctype that is not CRC32 or CRC32C (HDFS_CRC32C_CSUM_NULL has no CRCs
 * to combine).  Streams may overlap each other or be identical.
 *
 * ORDERING.  The work (one table upload, the probe, the fold and the reduce
 * launch, one copy of the tables back) is enqueued on `stream`, a hipStream_t
 * of the engine's device; NULL is a stream of this library that waits for the
 * NULL stream (a blocking stream): bytes written by other non-blocking streams
 * must then be complete before the call.  With a stream of the caller's, the
 * streams' bytes must be ordered ahead of the call on that stream:
 * hdfs_read_batch_read_blocks or hdfs_wire_fused_batch_compose followed at
 * once by this call with the same stream needs no synchronisation in between.
 * The call returns after the stream has been synchronised.  Entries handed to
 * hdfs_crc32c_parse_packets are framed after that synchronise, one by one,
 * under that call's own rules; their fold and reduce launches run on `stream`
 * again and are synchronised before return.  Calls from several threads are
 * serialised inside the library by one mutex (one device table and one pinned
 * staging area, the per-packet table of 4 bytes a packet and the fallback's
 * scratch, grown on demand and kept). */
int hdfs_crc_streams_block_crcs(hdfs_crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    void *stream);

/* hdfs_crc_streams_block_crcs, then the file's composite CRC on the host (with
 * hdfs_crc_streams_combine): e[0..n) are the file's blocks in order, *out gets
 * bytes_per_crc = chunk_size, ctype, the blocks' CRCs combined over their
 * payload lengths, its big-endian bytes and the sum of the payloads.  Returns
 * what the block CRCs return when that is negative; else HDFS_CRC32C_EINVAL,
 * with the entries' out fields filled and the text naming the entry, when out
 * is NULL or any entry has rc != 0 or offset_in_block != 0 (its stream does
 * not start at the block's start); else 0. */
int hdfs_crc_streams_file_checksum(hdfs_crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    void *stream, struct hdfs_crc_streams_file_checksum *out);

/* Host code that touches no device: *out = the CRC of n pieces in order, piece
 * i of lens[i] bytes with CRC crcs[i] (acc = acc * x^(8 lens[i]) ^ crcs[i],
 * from 0), for a caller whose file spans several calls.  n == 0 gives 0.  A
 * NULL out, NULL arrays with n > 0, or a ctype that is not CRC32 or CRC32C is
 * HDFS_CRC32C_EINVAL. */
int hdfs_crc_streams_combine(const uint32_t *crcs, const uint64_t *lens, size_t n, int ctype, uint32_t *out);

/* Measurement (tools/crc_streams_bench.py): hdfs_crc_streams_block_crcs once on
 * the library's stream, then the three launches alone iters more times between
 * two HIP events; *ms_per_iter is their distance over iters.  flags: none is
 * defined (HDFS_CRC_STREAMS_TIME_NONE); any flag bit, iters < 1 or a NULL
 * ms_per_iter is HDFS_CRC32C_EINVAL before any device is touched: as after every
 * refusal, the entries' out fields and *ms_per_iter (when given) are zero and
 * nothing else is written. */
#define HDFS_CRC_STREAMS_TIME_NONE 0u
int hdfs_crc_streams_time(hdfs_crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_CRC_STREAMS_H */
