/*
 * C consumer of the gather-write companion library (include/hadoofus_writev.h),
 * written the way hdfs_datanode_writev's call site would use it
 * (INTEGRATION.md): a write held in three device buffers at odd offsets of one
 * allocation -- a header blob and two payload buffers -- composed in place,
 * and, as a check, the same bytes packed into one buffer and composed by
 * hdfs_crc32c_compose_packets of the main library: the header buffers and the
 * packet records must be identical.
 * Prints the layout, the packet count and "0 failures" on success.
 * Test infrastructure (tests/test_writev_cpu.py links it on CPU,
 * tests/test_gpu_writev.py runs it on the GPU).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_writev.h"

#define NFRAG 3

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; writev: %s)\n", what, hdfs_crc32c_last_error(), hdfs_writev_last_error());
		failures++;
	}
}

int main(void)
{
	/* fragment i lives at off[i] of the arena; the gaps are never read */
	const uint64_t off[NFRAG] = { 3, 4096 + 1, 300000 + 2 }, len[NFRAG] = { 333, 200001, 70007 };
	const uint64_t arena_bytes = 400000, total = 333 + 200001 + 70007;
	const int64_t block_off = 4321, seqno = 17;
	void *arena = NULL, *packed = NULL;
	hdfs_crc32c_iovec iov[NFRAG];
	uint64_t lens[NFRAG], at = 0, used_v = 0, used_p = 0;
	size_t n_v = 0, n_p = 0;
	hdfs_writev_layout_info li;

	check(hdfs_writev_abi_version() == HDFS_WRITEV_ABI_VERSION, "abi version");
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0 && hdfs_crc32c_dev_alloc(&packed, total) == 0, "dev_alloc");
	check(hdfs_crc32c_fill_splitmix64(arena, arena_bytes / 8, 11, 0, NULL) == 0, "fill");
	for (int i = 0; i < NFRAG; i++) {
		iov[i].base = (uint8_t *)arena + off[i];
		iov[i].len = lens[i] = len[i];
		check(hdfs_crc32c_memcpy((uint8_t *)packed + at, iov[i].base, len[i], 2) == 0, "pack");
		at += len[i];
	}
	check(hdfs_writev_layout(lens, NFRAG, block_off, &li) == 0 && li.total == total &&
	    li.seg_chunks + li.ngathered == li.nchunks && li.nsegments == 2 && li.ngathered >= 3, "layout");
	printf("layout: %llu chunks, %llu segments over %llu chunks, %llu gathered from %llu pieces\n",
	    (unsigned long long)li.nchunks, (unsigned long long)li.nsegments, (unsigned long long)li.seg_chunks,
	    (unsigned long long)li.ngathered, (unsigned long long)li.npieces);

	/* size query, then the call */
	check(hdfs_writev_compose_packets(iov, NFRAG, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    NULL, 0, NULL, 0, &n_v, &used_v) == 0 && n_v > 0 && used_v > 0, "size query");
	uint8_t *hdr_v = malloc(used_v), *hdr_p = malloc(used_v);
	hdfs_crc32c_out_packet *pk_v = calloc(n_v, sizeof(*pk_v)), *pk_p = calloc(n_v, sizeof(*pk_p));
	check(hdfs_writev_compose_packets(iov, NFRAG, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    hdr_v, used_v, pk_v, n_v, &n_v, &used_v) == 0, "writev compose");
	check(hdfs_crc32c_compose_packets(packed, total, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    hdr_p, used_v, pk_p, n_v, &n_p, &used_p) == 0, "packed compose");
	check(n_p == n_v && used_p == used_v, "same sizes");
	check(memcmp(hdr_v, hdr_p, used_v) == 0, "header buffers identical");
	check(memcmp(pk_v, pk_p, n_v * sizeof(*pk_v)) == 0, "packet records identical");
	printf("%zu packets, %llu header bytes\n", n_v, (unsigned long long)used_v);

	/* a host fragment among device fragments is refused */
	uint8_t hostbuf[64] = { 0 };
	iov[1].base = hostbuf;
	iov[1].len = sizeof(hostbuf);
	check(hdfs_writev_compose_packets(iov, NFRAG, 0, 0, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 0, hdr_v, used_v,
	    pk_v, n_v, &n_v, &used_v) == HDFS_CRC32C_EINVAL, "mixed fragments refused");

	free(hdr_v);
	free(hdr_p);
	free(pk_v);
	free(pk_p);
	hdfs_crc32c_dev_free(packed);
	hdfs_crc32c_dev_free(arena);
	printf("%d failures\n", failures);
	return failures != 0;
}
