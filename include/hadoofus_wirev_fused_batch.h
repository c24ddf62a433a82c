/*
 * hadoofus_wirev_fused_batch.h -- the wire streams of a batch of writes, each
 * held in a list of device buffers, in one call, one launch and ONE pass over
 * the data (libhadoofus_wirev_fused_batch.so, a companion of
 * libhadoofus_crc32c.so built from hadoofus_amd/csrc/wirev_fused_batch*).
 *
 * The reference's write entry points take an iovec array
 * (hdfs_datanode_writev / hdfs_datanode_writev_nb), and a datanode that keeps
 * many pipelines busy has many small gather writes outstanding at once.
 * hdfs_wirev_fused_compose_packets (hadoofus_wirev_fused.h) reads such a
 * write's fragments once but takes one write per call: every call pays a table
 * upload, a launch, a synchronise and a 156 KiB table fill per workgroup.
 * hdfs_wire_fused_batch_compose (hadoofus_wire_fused_batch.h) pays that once
 * per batch but wants every write contiguous.  This library's kernel,
 * frame_fused_gather_batch_kernel, runs the fused kernel's round over the
 * packets of all writes of a batch and finds every round's bytes through one
 * fragment table: one upload, one launch, one synchronise, the table image
 * filled once per workgroup, no compute plan, no CRC array and no packing pass.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  At every shape measured, against the one way of doing the job
 * without it that reads the data once: a loop of
 * hdfs_wirev_fused_compose_packets calls.  One MI355X
 * (tools/wirev_fused_batch_bench.py; medians of 5
 * (min-max) per write with the three paths alternated in one process after two
 * warm-ups of each, host clock around each whole path, which ends in its
 * synchronise, block offset 4321, CRC32C, v2, finish, every fragment a range
 * of its own at an odd address, every stream of all three paths downloaded and
 * compared; two runs of the command, the first run's figures), microseconds
 * per write.  "floor" is hdfs_wire_fused_batch_compose on the same bytes
 * already packed contiguously, the packing not timed: no caller has that for
 * free; it shows what the fragment table and the seams cost.
 *     writes x size in fragments         this call            gather loop          floor
 *       16 x 128 MiB in   16 x 8 MiB     76.8 (76.4-82.1)     104.6 (104.2-105.5)  76.2 (75.1-76.5)
 *       16 x 128 MiB in 1024 x 128 KiB   97.1 (96.5-100.5)    116.7 (116.3-117.6)  75.7 (74.9-76.3)
 *       64 x   1 MiB in   16 x 64 KiB    1.32 (1.31-1.39)     29.0 (28.9-29.1)     1.03 (1.03-1.07)
 *     1024 x  64 KiB in   16 x 4 KiB     0.252 (0.243-0.281)  29.8 (29.7-29.9)     0.173 (0.169-0.192)
 *     1024 x  64 KiB in    1             0.166 (0.158-0.175)  26.4 (26.4-26.5)     0.175 (0.165-0.183)
 *     4096 x   4 KiB in    3 x 1365 B    0.167 (0.165-0.176)  27.4 (27.4-27.5)     0.174 (0.165-0.177)
 *       64 x   8 MiB in 2049 x 4097 B    18.4 (18.3-19.6)     46.6 (46.4-46.7)     5.30 (5.26-5.45)
 * This call's range lies below the loop's in all seven rows, in both runs: 1.2
 * to 1.4 times for 128 MiB writes (the per-call launch and synchronise), 2.5
 * times for 8 MiB writes in 2 049 fragments, 22 to 165 times for writes of
 * 1 MiB and less, where the loop pays 26 to 30 us per call whatever the size.
 * Against the floor it is no difference shown with 16 fragments of 8 MiB, with
 * one fragment and with three per 4 KiB write, and SLOWER wherever many rounds
 * are seamed or the host walks many fragments: 1.28 times with 1 024 fragments
 * per 128 MiB (the kernel alone takes 76 against 61 us per write, the rest is
 * the host's pass over 16 384 fragments), 1.28 times for 64 x 1 MiB in 16, 1.46
 * times for 64 KiB writes in 16 fragments of 4 KiB (15 of every 16 rounds
 * seamed), 3.5 times for 8 MiB in 2 049 fragments (nearly every round seamed: the
 * kernel alone 5.9 against 3.9 us per write, the host 12 us per write for its
 * fragments: their sum, their places, the overlap sweep, the table).  A caller
 * whose bytes are contiguous already should call hdfs_wire_fused_batch_compose.
 * Not measured: CRC32, v1, CSUM_NULL, a caller's stream, block offset 0,
 * batches of mixed sizes, fragment lists that do not rise in address (the host
 * then sorts every fragment's range for the overlap sweep), packing the
 * fragments first as a timed path.
 *
 * A wave walks the fragments under a seamed round one after the other, as in
 * hadoofus_wirev_fused.h: a round made of thousands of one-byte fragments is
 * framed correctly but slowly.  A workgroup takes one packet a step, as in
 * hadoofus_wire_fused_batch.h: a caller who can present many tiny writes as
 * one should.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_wirev_fused_batch_last_error()).
 */
#ifndef HADOOFUS_WIREV_FUSED_BATCH_H
#define HADOOFUS_WIREV_FUSED_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_WIREV_FUSED_BATCH_<n>
 * (hadoofus_amd/csrc/wirev_fused_batch_exports.map); run-time bindings compare
 * hdfs_wirev_fused_batch_abi_version() with the version they were written for.
 * The main library's ABI version and the other companions' are not affected. */
#define HDFS_WIREV_FUSED_BATCH_ABI_VERSION 1

/* Most writes in one call, and most non-empty fragments of all writes of a call. */
#define HDFS_WIREV_FUSED_BATCH_MAX_WRITES 65536
#define HDFS_WIREV_FUSED_BATCH_MAX_FRAGS  (1u << 22)

int hdfs_wirev_fused_batch_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_wirev_fused_batch_last_error(void);

/* One write of a batch: hdfs_wirev_fused_compose_packets' arguments of it, and
 * what the call reports back about it. */
typedef struct hdfs_wirev_fused_batch_write {
	const hdfs_crc32c_iovec *iov; /* host array of iovcnt device fragments, any alignment, any length */
	int32_t     iovcnt;       /* may be 0 */
	int32_t     finish;       /* != 0: the empty lastPacketInBlock packet ends the write */
	int64_t     offset_in_block;
	int64_t     seqno;        /* of the write's first packet */
	void       *wire;         /* device, any alignment; NULL in every entry = size query */
	uint64_t    wire_cap;     /* bytes of room at wire */
	/* out */
	uint64_t    len;          /* sum of the fragments' lengths, at most 1 TiB */
	uint64_t    wire_len;     /* bytes of this write's stream */
	uint64_t    npkts;        /* its packets */
	uint64_t    first_pkt;    /* index of its first record in pkts */
} hdfs_wirev_fused_batch_write;

/* The streams of the nwrites writes w[0..nwrites): after a successful call
 * w[k].wire[0, w[k].wire_len) is byte for byte what
 * hdfs_wirev_fused_compose_packets writes for (iov, iovcnt, offset_in_block,
 * seqno, proto, ctype, finish) of entry k -- hdfs_wire_compose_packets' stream
 * of the fragments' concatenation -- and the records pkts[w[k].first_pkt ..
 * first_pkt + npkts) (pkts may be NULL) equal that call's records, hdr_off
 * counting inside write k's own stream, data_off in its concatenation.  The
 * records lie in batch order; *npkts is their total.  proto and ctype hold for
 * the whole batch; HDFS_CRC32C_CSUM_NULL does no CRC work and still frames
 * headers and data.  An empty write with finish is one header-only packet; an
 * empty write without it is no packet and no work, and may sit anywhere in the
 * batch.
 *
 * Fragments are device memory of the engine's device, each inside one device
 * allocation, at any byte alignment and of any length.  Zero-length fragments
 * are allowed anywhere (base may then be NULL) and iovcnt may be 0.  Fragments
 * may overlap each other, repeat and come in any address order, within one
 * entry and across entries (two replicas of one block).  Every wire range is
 * device memory of the same device inside one allocation; no wire range may
 * overlap another wire range or any fragment of any entry.
 *
 * Each of these is HDFS_CRC32C_EINVAL for the whole call with nothing written
 * anywhere, the out fields of every entry and *npkts still set, and the error
 * text naming the offending entry's index ("entry <k>") and, where a fragment
 * is at fault, the fragment's ("fragment <i>"): a negative iovcnt, a NULL iov
 * with iovcnt > 0, a NULL base with a length, a host or mixed fragment list, a
 * fragment or wire range that leaves its allocation, a wire range over another
 * wire range or over any fragment of any entry, wire_cap < wire_len, (with
 * pkts) max_pkts smaller than *npkts, and some entries with wire == NULL while
 * others have one.  (A negative iovcnt, a NULL iov and the limits below are
 * judged before any write is laid out: the out fields are then zero.)  If every
 * wire is NULL the call is a size query that touches no device and reads only
 * the fragments' lengths, never a base: the out fields and *npkts are set, and
 * the records too when pkts has room.
 *
 * At most HDFS_WIREV_FUSED_BATCH_MAX_WRITES writes,
 * HDFS_WIREV_FUSED_BATCH_MAX_FRAGS non-empty fragments in all, 1 TiB per
 * write and (2^31 - 1) / 4 packets in all; each is refused in closed form,
 * before any write's packets are walked.
 *
 * Only the fragments' own bytes are read -- not the aligned words around
 * them: every vector access goes through a buffer descriptor over exactly the
 * bytes it may touch -- and only the wire ranges [wire, wire + wire_len) are
 * written, every byte of them once.
 *
 * ORDERING.  The work (one table upload, then one kernel) is enqueued on
 * `stream`, a hipStream_t of the engine's device; NULL is a stream of this
 * library that waits for the NULL stream (a blocking stream): bytes written by
 * other non-blocking streams must then be complete before the call.  With a
 * stream of the caller's, the data must be ordered ahead of the call on that
 * stream.  The call returns after the stream has been synchronised: the
 * streams' bytes are then visible to every later operation on the device.
 * Calls from several threads are serialised inside the library by one mutex
 * (the CRC tables, uploaded once per device and kept; one device table and one
 * pinned staging area, grown on demand and kept). */
int hdfs_wirev_fused_batch_compose(hdfs_wirev_fused_batch_write *w, size_t nwrites, int proto, int ctype,
    hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, void *stream);

/* Host only, no GPU: fills the out fields of every entry (wire and wire_cap are
 * not looked at; the fragments' lengths are read, never a base) and the totals
 * of the batch: hdfs_wire_fused_batch_totals' four, then which of the kernel's
 * paths the batch's rounds take, as hdfs_wirev_fused_layout counts them for
 * each write. */
typedef struct hdfs_wirev_fused_batch_totals {
	uint64_t npkts;          /* packets of all writes */
	uint64_t nchunks;        /* chunks of all writes (CRCs computed unless CSUM_NULL) */
	uint64_t wire_bytes;     /* sum of the streams' lengths */
	uint64_t table_entries;  /* writes with at least one packet: entries of the device's write table */
	uint64_t nfrags;         /* non-empty fragments of all writes */
	uint64_t rounds;         /* 4 KiB rounds with at least one full chunk */
	uint64_t seamed_rounds;  /* those whose full chunks do not lie inside one fragment */
	uint64_t seamed_ragged;  /* chunks shorter than 512 B that do not */
	uint32_t max_frags_per_round; /* most non-empty fragments under one round's full chunks */
	uint32_t reserved;
} hdfs_wirev_fused_batch_totals;
int hdfs_wirev_fused_batch_layout(hdfs_wirev_fused_batch_write *w, size_t nwrites, int proto, int ctype,
    hdfs_wirev_fused_batch_totals *out);

/* Measurement (tools/wirev_fused_batch_bench.py):
 * hdfs_wirev_fused_batch_compose once on the library's stream, then
 * frame_fused_gather_batch_kernel alone iters more times between two HIP
 * events; *ms_per_iter is their distance over iters.  flags:
 * HDFS_WIREV_FUSED_BATCH_TIME_GROUPS(n) launches n workgroups (1..1024)
 * instead of the product's grid (one per compute unit, at most one per
 * packet), so that every workgroup walks many packets across the writes; any
 * other flag bit, n above 1024, iters < 1 or a NULL ms_per_iter is
 * HDFS_CRC32C_EINVAL before any device is touched, with nothing written.  The
 * streams written are the same under every flag. */
#define HDFS_WIREV_FUSED_BATCH_TIME_GROUPS(n) ((unsigned)(n) << 8)
int hdfs_wirev_fused_batch_time(hdfs_wirev_fused_batch_write *w, size_t nwrites, int proto, int ctype,
    unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_WIREV_FUSED_BATCH_H */
