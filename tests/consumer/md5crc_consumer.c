/*
 * C consumer of the MD5CRC companion library (include/hadoofus_md5crc.h),
 * written the way a datanode's OP_BLOCK_CHECKSUM handler and a client's
 * getFileChecksum would use it: three blocks of a file in
 * device memory (allocated and filled through the main library), one compute
 * plan for their chunk CRCs, then the block digests and the file checksum
 * from the CRC arrays -- the data is not read again and the CRCs do not leave
 * the device.  As a check it downloads the CRCs once and digests them on the
 * host (hdfs_md5crc_md5_host; they are in wire order already).
 * Prints each block digest, the file checksum and "0 failures" on success.
 * Test infrastructure (tests/test_md5crc_cpu.py links it on CPU,
 * tests/test_gpu_md5crc.py runs it on the GPU).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_md5crc.h"

#define NBLK 3
#define CS 512u

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; md5crc: %s)\n", what, hdfs_crc32c_last_error(), hdfs_md5crc_last_error());
		failures++;
	}
}

static void print_hex(const char *label, const uint8_t *p, size_t n)
{
	printf("%s", label);
	for (size_t i = 0; i < n; i++)
		printf("%02x", p[i]);
	printf("\n");
}

int main(void)
{
	/* two full 1 MiB blocks and a short last block with a partial chunk */
	const uint64_t blen[NBLK] = { 1u << 20, 1u << 20, 300 * CS + 77 };
	hdfs_crc32c_segment seg[NBLK];
	void *data[NBLK], *crcs[NBLK];
	uint8_t md5[NBLK][HDFS_MD5CRC_LEN], want[HDFS_MD5CRC_LEN], wire[HDFS_MD5CRC_FILE_BYTES];
	hdfs_md5crc_file_checksum fc, fc2;
	hdfs_crc32c_plan *plan = NULL;
	char name[64];

	check(hdfs_md5crc_abi_version() == HDFS_MD5CRC_ABI_VERSION, "abi version");
	memset(seg, 0, sizeof(seg));
	for (int b = 0; b < NBLK; b++) {
		const uint64_t nch = (blen[b] + CS - 1) / CS, words = (blen[b] + 7) / 8;
		check(hdfs_crc32c_dev_alloc(&data[b], words * 8) == 0 && hdfs_crc32c_dev_alloc(&crcs[b], nch * 4) == 0,
		    "dev_alloc");
		check(hdfs_crc32c_fill_splitmix64(data[b], words, 7, (uint64_t)b << 20, NULL) == 0, "fill");
		seg[b].data = data[b];
		seg[b].len = blen[b];
		seg[b].chunk_size = CS;
		seg[b].flags = HDFS_CRC32C_SEG_BE;
		seg[b].crcs = crcs[b];
	}
	check(hdfs_crc32c_plan_create(&plan, HDFS_CRC32C_MODE_COMPUTE, seg, NBLK) == 0, "plan_create");
	/* the plan and the digests on the same (NULL) stream: no sync in between */
	check(hdfs_crc32c_plan_execute(plan, NULL) == 0, "plan_execute");
	check(hdfs_md5crc_block_digests(seg, NBLK, NULL, md5) == 0, "block_digests");
	check(hdfs_md5crc_file_checksum_dev(seg, NBLK, NULL, &fc) == 0, "file_checksum_dev");

	for (int b = 0; b < NBLK; b++) {
		const uint64_t nch = (blen[b] + CS - 1) / CS;
		uint8_t *h = malloc(nch * 4);
		check(hdfs_crc32c_memcpy(h, crcs[b], nch * 4, 1) == 0, "download crcs");
		check(hdfs_md5crc_md5_host(h, nch * 4, want) == 0 && memcmp(want, md5[b], HDFS_MD5CRC_LEN) == 0,
		    "block digest == host MD5 of the wire-order CRCs");
		free(h);
		print_hex("block ", md5[b], HDFS_MD5CRC_LEN);
	}
	check(hdfs_md5crc_file_from_blocks(md5, NBLK, CS, (1u << 20) / CS, HDFS_CRC32C_CSUM_CRC32C, &fc2) == 0,
	    "file_from_blocks");
	check(fc.bytes_per_crc == CS && fc.crc_per_block == (1u << 20) / CS && fc.ctype == HDFS_CRC32C_CSUM_CRC32C &&
	    memcmp(fc.md5, fc2.md5, HDFS_MD5CRC_LEN) == 0, "file checksum fields");
	check(hdfs_md5crc_algorithm_name(&fc, name, sizeof(name)) == 0 &&
	    strcmp(name, "MD5-of-2048MD5-of-512CRC32C") == 0, "algorithm name");
	check(hdfs_md5crc_file_bytes(&fc, wire) == 0 && wire[2] == 2 && wire[10] == 8 &&
	    memcmp(wire + 12, fc.md5, HDFS_MD5CRC_LEN) == 0, "file bytes");
	printf("file %s:", name);
	print_hex("", fc.md5, HDFS_MD5CRC_LEN);

	/* a raw-register segment has no MD5CRC */
	seg[0].flags |= HDFS_CRC32C_SEG_RAW;
	check(hdfs_md5crc_block_digests(seg, 1, NULL, md5) == HDFS_CRC32C_EINVAL, "SEG_RAW refused");

	hdfs_crc32c_plan_destroy(plan);
	for (int b = 0; b < NBLK; b++) {
		hdfs_crc32c_dev_free(crcs[b]);
		hdfs_crc32c_dev_free(data[b]);
	}
	printf("%d failures\n", failures);
	return failures != 0;
}
