/*
 * hadoofus_wirev_fused.h -- a write held in a list of device buffers as one
 * wire stream in device memory, in ONE pass over the data
 * (libhadoofus_wirev_fused.so, a companion of libhadoofus_crc32c.so built from
 * hadoofus_amd/csrc/wirev_fused*).
 *
 * The reference's write entry points take an iovec array
 * (hdfs_datanode_writev / hdfs_datanode_writev_nb) and chain every 512-B
 * chunk's CRC across fragment boundaries (src/datanode.c:2836-2859).
 * hdfs_wirev_compose_packets (hadoofus_wirev.h) makes such a write's stream in
 * two passes: a compute plan of the main library over the runs of whole chunks
 * and a kernel over every chunk that crosses a fragment boundary leave the
 * CRCs in a scratch array, two tables go up, and a frame kernel reads the
 * fragments again.  This library's kernel, frame_fused_gather_kernel, reads
 * the fragments once: it is the kernel of hadoofus_wire_fused.h with a table
 * of the fragments for a data source.  A 4 KiB round whose bytes lie in one
 * fragment is that kernel's round; a round with a fragment boundary inside is
 * assembled into the same registers piece by piece, then stored and
 * checksummed by the same code.  There is no compute plan, no CRC array, no
 * gather table and one launch.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library.
 *
 * WHEN IT PAYS.  At every shape measured, against hdfs_wirev_compose_packets
 * on the same fragments, when the call is timed alone; there is no fragment
 * size down to 4 000 B below which the two-pass call remains the one to use
 * (smaller fragments were not measured).  One MI355X
 * (tools/wirev_fused_bench.py; medians of 5 (min-max),
 * host clock around each whole call, which ends in its synchronise, CRC32C, v2,
 * finish, fragments at odd addresses, all buffers allocated beforehand, all
 * streams downloaded and compared; two runs of the command, the first run's
 * figures).  "alternated": this call, the two-pass call (and with one fragment
 * hdfs_wire_fused_compose_packets) taking turns in one process after a warm-up
 * of each; "alone": the same call back to back.
 *     write    fragments      offset  alternated: this call / two-pass call        alone: this call / two-pass call
 *     128 MiB      1              0   0.090 (0.090-0.092) / 0.146 (0.144-0.149)    0.090 (0.089-0.090) / 0.146 (0.145-0.148)
 *     128 MiB      1           4321   0.083 (0.080-0.088) / 0.183 (0.177-0.192)    0.082 (0.080-0.082) / 0.194 (0.189-0.210)
 *     128 MiB     16 x 8 MiB   4321   0.149 (0.136-0.191) / 0.239 (0.222-0.340)    0.098 (0.096-0.107) / 0.277 (0.234-0.323)
 *     128 MiB    128 x 1 MiB   4321   0.121 (0.106-0.134) / 0.233 (0.228-0.241)    0.098 (0.097-0.099) / 0.227 (0.226-0.238)
 *     128 MiB  1 024 x 128 KiB 4321   0.134 (0.123-0.140) / 0.370 (0.370-0.374)    0.108 (0.106-0.109) / 0.391 (0.372-0.415)
 *     128 MiB 16 383 x 8 193 B 4321   0.157 (0.157-0.170) / 2.441 (2.433-2.450)    0.155 (0.153-0.156) / 2.435 (2.435-2.445)
 *     128 MiB 33 555 x 4 000 B 4321   0.220 (0.214-0.233) / 1.610 (1.585-1.685)    0.205 (0.204-0.205) / 1.626 (1.597-2.031)
 *       1 GiB     64 x 16 MiB  4321   0.791 (0.758-1.893) / 0.974 (0.828-2.459)    0.729 (0.725-0.734) / 0.863 (0.862-0.869)
 *       1 MiB      1           4321   0.028 (0.028-0.030) / 0.103 (0.102-0.108)    0.027 (0.027-0.028) / 0.108 (0.107-0.115)
 *       1 MiB     16 x 64 KiB  4321   0.035 (0.034-0.035) / 0.120 (0.118-0.120)    0.030 (0.030-0.030) / 0.123 (0.122-0.125)
 *       8 MiB      1           4321   0.032 (0.031-0.048) / 0.114 (0.109-0.123)    0.030 (0.030-0.031) / 0.113 (0.111-0.117)
 *       8 MiB     16 x 512 KiB 4321   0.035 (0.035-0.040) / 0.122 (0.120-0.126)    0.030 (0.030-0.031) / 0.125 (0.123-0.126)
 * (ms).  Alone, the two ranges are clear of each other in all twelve rows in
 * both runs: 1.6 to 3.6 times faster for 128 MiB in up to 1 024 fragments, 8 to
 * 16 times with thousands of fragments (no gather layout, no gathered-chunk
 * kernel, no second read), 3.7 to 4.2 times up to 8 MiB (fixed cost: no plan,
 * one launch), 1.18 times at 1 GiB.  Alternated, nine rows are faster in both
 * runs; the 1 GiB row overlapped in the first run (no difference shown there,
 * faster in the second); and the two rows with thousands of fragments were
 * faster in the first run and SLOWER in the second, in which the two-pass call
 * alone took 20 to 30 ms instead of 1.6 to 2.4 and this call, when it came
 * right behind one, 14 to 26 ms instead of 0.16 to 0.23: the call that follows
 * such a two-pass call pays for something that call leaves behind (not taken
 * apart; this call alone stayed at 0.15-0.19 and 0.20-0.23 ms in every run).
 * With one fragment the call alone costs what hdfs_wire_fused_compose_packets
 * costs at 128 MiB (no difference shown: 0.089-0.090 against 0.088-0.089 ms)
 * and about 3 us more at 1 MiB (0.027-0.028 against 0.024-0.025 ms): the table's
 * upload.  The kernel alone (HIP events around ten launches) takes 52 to 60 us
 * for 128 MiB in one fragment, as the single-write fused kernel does, 65 to 69
 * us in 16 to 1 024 fragments, 78 us with 8 193-B and 84 us with 4 000-B
 * fragments, where every round has a fragment boundary inside; the two-pass
 * library's frame kernel alone, its CRC pass not counted, takes 47 to 54, 96
 * and 142 us.  Not measured: CRC32, v1, CSUM_NULL, a caller's stream,
 * fragments below 4 000 B, writes between 8 and 128 MiB and above 1 GiB.
 *
 * A wave walks the fragments under a seamed round one after the other, one
 * scalar round trip and up to 36 vector loads per piece: a round made of
 * thousands of one-byte fragments is framed correctly but slowly, as in
 * hadoofus_wirev.h.  There is no second mapping for such writes.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_wirev_fused_last_error()).
 */
#ifndef HADOOFUS_WIREV_FUSED_H
#define HADOOFUS_WIREV_FUSED_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_WIREV_FUSED_<n>
 * (hadoofus_amd/csrc/wirev_fused_exports.map); run-time bindings compare
 * hdfs_wirev_fused_abi_version() with the version they were written for.  The
 * main library's ABI version is not affected by this one. */
#define HDFS_WIREV_FUSED_ABI_VERSION 1

int hdfs_wirev_fused_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_wirev_fused_last_error(void);

/* Same arguments in the same order, same contract, same records, same bytes
 * as hdfs_wirev_compose_packets (hadoofus_wirev.h): after a successful call
 * wire[0, *wire_len) is byte for byte what hdfs_wire_compose_packets writes
 * for the fragments' concatenation, and the records in pkts (may be NULL) are
 * that call's: hdr_off counts in the stream, data_off in the concatenation.
 * Packet sizing, finish, proto, ctype, offset_in_block and seqno are
 * hdfs_crc32c_compose_packets'.  HDFS_CRC32C_CSUM_NULL does no CRC work and
 * still frames headers and data.
 *
 * Fragments are device memory of the engine's device, each inside one device
 * allocation, at any byte alignment and of any length; zero-length fragments
 * are allowed anywhere (base may then be NULL); fragments may overlap each
 * other, come in any address order and repeat.  wire is device memory of the
 * same device, [wire, wire + *wire_len) inside one allocation and clear of
 * every fragment.  A host or mixed fragment list, a fragment that runs past
 * its allocation, a NULL base with a length, a wire range outside one
 * allocation or over a fragment, wire_cap < *wire_len and (with pkts)
 * max_pkts < *npkts are HDFS_CRC32C_EINVAL with nothing written, *npkts and
 * *wire_len still set; the text names the fragment ("fragment <i>").
 * wire == NULL is a size query that touches no device and reads only the
 * fragments' lengths: *npkts and *wire_len are set, and the records too when
 * pkts has room.  An empty write with finish is one header-only packet; an
 * empty write without it is no packet and no work.  At most 1 TiB per call
 * and fewer than 2^32 - 1 non-empty fragments.
 *
 * Only the fragments' own bytes are read -- not the aligned words around
 * them: every vector access goes through a buffer descriptor over exactly the
 * bytes it may touch -- and only [wire, wire + *wire_len) is written, every
 * byte of it once.
 *
 * ORDERING.  As hdfs_wire_fused_compose_packets: the work (the fragment
 * table's upload, then the kernel) is enqueued on `stream`, a hipStream_t of
 * the engine's device; NULL is a stream of this library that waits for the
 * NULL stream (a blocking stream): bytes written by other non-blocking streams
 * must then be complete before the call.  With a stream of the caller's, the
 * fragments' bytes must be ordered ahead of the call on that stream.  The call
 * returns after the stream has been synchronised: the stream's bytes are then
 * visible to every later operation on the device.  Calls from several threads
 * are serialised inside the library by one mutex, held from the table's upload
 * to that synchronise (the CRC tables, uploaded once per device, and one
 * fragment table, grown on demand, are kept). */
int hdfs_wirev_fused_compose_packets(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block,
    int64_t seqno, int proto, int ctype, int finish, void *wire, uint64_t wire_cap, hdfs_crc32c_out_packet *pkts,
    size_t max_pkts, size_t *npkts, uint64_t *wire_len, void *stream);

/* Host only, no GPU: the shape of the stream of a write of these fragment
 * lengths, as hdfs_wirev_layout reports it, and which of the kernel's paths
 * its rounds take.  A round is 4 KiB (eight chunks) of a packet's full
 * chunks, counted from the packet's first data byte; a packet's chunk shorter
 * than 512 B (the short first packet, the write's last chunk) is no round. */
typedef struct hdfs_wirev_fused_layout_info {
	uint64_t npkts;          /* packets, the empty last one of `finish` included */
	uint64_t nchunks;        /* chunks on the write's chunk grid (CRCs computed unless CSUM_NULL) */
	uint64_t wire_len;       /* bytes of the stream */
	uint64_t nfrags;         /* non-empty fragments: entries of the kernel's table */
	uint64_t rounds;         /* rounds with at least one full chunk */
	uint64_t seamed_rounds;  /* those whose full chunks do not lie inside one fragment */
	uint64_t seamed_ragged;  /* chunks shorter than 512 B that do not */
	uint32_t packet_stride;  /* bytes of a full 64 KiB packet: 66 079 (v2) / 66 073 (v1) with checksums */
	uint32_t header_bytes;   /* bytes ahead of a packet's CRCs: 31 (v2) / 25 (v1) */
	uint32_t head_bytes;     /* data bytes of the short first packet (0: none) */
	uint32_t max_frags_per_round; /* most non-empty fragments under one round's full chunks */
} hdfs_wirev_fused_layout_info;
int hdfs_wirev_fused_layout(const uint64_t *lens, int iovcnt, int64_t offset_in_block, int proto, int ctype,
    int finish, hdfs_wirev_fused_layout_info *out);

/* Measurement (tools/wirev_fused_bench.py): hdfs_wirev_fused_compose_packets
 * once, then the kernel alone iters more times on the library's stream between
 * two HIP events; *ms_per_iter is their distance over iters.  flags:
 * HDFS_WIREV_FUSED_TIME_GROUPS(n) launches n workgroups (1..1024) instead of
 * the product's grid (one per compute unit, at most one per packet), so that
 * every workgroup walks many packets; any other flag bit, or n above 1024, is
 * HDFS_CRC32C_EINVAL with nothing written.  Every argument error is reported
 * before a device is touched.  The stream written is the same under every
 * flag. */
#define HDFS_WIREV_FUSED_TIME_GROUPS(n) ((unsigned)(n) << 8)
int hdfs_wirev_fused_time(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block, int proto, int ctype,
    int finish, void *wire, uint64_t wire_cap, unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_WIREV_FUSED_H */
