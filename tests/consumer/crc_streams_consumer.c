/*
 * C consumer of the CRC streams library (include/hadoofus_crc_streams.h),
 * written the way a client that has just read a file of several blocks into
 * GPU memory would use it: three blocks' packet streams (v2, CRC32C; 4 KiB
 * packets, a shorter one, the empty last one), built on the host with a
 * bitwise CRC of this file's own and uploaded at odd addresses of one device
 * allocation, give their composite CRCs and the file's in one call.  The
 * framing outputs are checked against what the streams were built from, the
 * CRCs against the bitwise CRC of the payloads and of their concatenation;
 * they are printed ("block <crc> <bytes>", "file <crc> <bytes>") for the test
 * that runs this.  One header bit flipped sends one entry, and only that one,
 * down the main library's path with the same CRC.
 * Prints "0 failures" on success.
 * Test infrastructure (tests/test_crc_streams_cpu.py links it on CPU,
 * tests/test_gpu_crc_streams.py runs it on the GPU).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_crc_streams.h"

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; crc streams: %s)\n", what, hdfs_crc32c_last_error(),
		    hdfs_crc_streams_last_error());
		failures++;
	}
}

static uint32_t crc32c_bitwise(uint32_t crc, const uint8_t *p, size_t n)
{
	uint32_t c = ~crc;
	while (n--) {
		c ^= *p++;
		for (int k = 0; k < 8; k++)
			c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
	}
	return ~c;
}

static uint8_t *put_be(uint8_t *p, uint64_t v, int n)
{
	for (int i = n - 1; i >= 0; i--)
		*p++ = (uint8_t)(v >> (8 * i));
	return p;
}

static uint8_t *put_le(uint8_t *p, uint64_t v, int n)
{
	for (int i = 0; i < n; i++)
		*p++ = (uint8_t)(v >> (8 * i));
	return p;
}

/* One v2 packet of dlen bytes of data at p.  Returns its end. */
static uint8_t *put_packet(uint8_t *p, const uint8_t *data, uint32_t dlen, int64_t off, int64_t seq, int last)
{
	const uint32_t ncrc = (dlen + 511) / 512;
	p = put_be(p, dlen + 4 * ncrc + 4, 4);
	p = put_be(p, 25, 2);
	*p++ = 0x09;
	p = put_le(p, (uint64_t)off, 8);
	*p++ = 0x11;
	p = put_le(p, (uint64_t)seq, 8);
	*p++ = 0x18;
	*p++ = (uint8_t)last;
	*p++ = 0x25;
	p = put_le(p, dlen, 4);
	for (uint32_t c = 0; c < ncrc; c++) {
		const uint32_t n = dlen - 512 * c < 512 ? dlen - 512 * c : 512;
		p = put_be(p, crc32c_bitwise(0, data + 512 * c, n), 4);
	}
	if (dlen)
		memcpy(p, data, dlen);
	return p + dlen;
}

#define NB 3

int main(void)
{
	const uint32_t full = 4096, nfull[NB] = { 5, 1, 9 }, tail[NB] = { 700, 0, 513 };
	const int V2 = HDFS_CRC32C_PROTO_V2, C = HDFS_CRC32C_CSUM_CRC32C;
	const size_t arena_bytes = 1 << 20, room = 80000;
	uint8_t *host = calloc(1, arena_bytes), *back = malloc(arena_bytes);
	void *arena = NULL;
	hdfs_crc_streams_entry e[NB];
	struct hdfs_crc_streams_file_checksum fc;
	uint64_t payload[NB], slen[NB], nchunks[NB], lens[NB];
	uint32_t want[NB], crcs[NB], whole = 0, combined = 7;

	check(hdfs_crc_streams_abi_version() == HDFS_CRC_STREAMS_ABI_VERSION, "abi version");
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0, "dev_alloc");
	memset(e, 0, sizeof(e));
	for (int b = 0; b < NB; b++) {
		uint8_t *s = host + 3 + b * 2 * room, *p = s;
		uint8_t *data;
		int64_t off = 0, seq = 0;
		payload[b] = (uint64_t)nfull[b] * full + tail[b];
		nchunks[b] = (uint64_t)nfull[b] * (full / 512) + (tail[b] + 511) / 512;
		data = malloc(payload[b]);
		for (uint64_t i = 0; i < payload[b]; i++)
			data[i] = (uint8_t)((i * 2654435761u + 97 * b) >> 7);
		want[b] = crc32c_bitwise(0, data, payload[b]);
		whole = crc32c_bitwise(whole, data, payload[b]);
		for (uint32_t k = 0; k < nfull[b]; k++, off += full)
			p = put_packet(p, data + off, full, off, seq++, 0);
		if (tail[b])
			p = put_packet(p, data + off, tail[b], off, seq++, 0);
		p = put_packet(p, NULL, 0, (int64_t)payload[b], seq, 1);
		slen[b] = (uint64_t)(p - s);
		e[b].stream = (uint8_t *)arena + (s - host);
		e[b].len = slen[b];
		free(data);
	}
	check(hdfs_crc32c_memcpy(arena, host, arena_bytes, 0) == 0, "upload");

	/* the call */
	check(hdfs_crc_streams_file_checksum(e, NB, V2, 512, C, NULL, &fc) == 0, "file_checksum");
	for (int b = 0; b < NB; b++) {
		const uint64_t np = nfull[b] + (tail[b] ? 1 : 0) + 1;
		check(e[b].rc == 0 && e[b].path == HDFS_CRC_STREAMS_PATH_KERNEL && e[b].npkts == np &&
		    e[b].consumed == slen[b] && e[b].payload == payload[b] && e[b].nchunks == nchunks[b] &&
		    e[b].offset_in_block == 0 && e[b].reserved == 0, "an entry's outputs");
		check(e[b].crc == want[b], "a block's CRC is its payload's");
		crcs[b] = e[b].crc;
		lens[b] = e[b].payload;
		printf("block %08x %llu\n", e[b].crc, (unsigned long long)e[b].payload);
	}
	check(fc.bytes_per_crc == 512 && fc.ctype == (uint32_t)C && fc.crc == whole &&
	    fc.length == payload[0] + payload[1] + payload[2], "the file checksum's fields");
	check(fc.bytes[0] == (uint8_t)(whole >> 24) && fc.bytes[1] == (uint8_t)(whole >> 16) &&
	    fc.bytes[2] == (uint8_t)(whole >> 8) && fc.bytes[3] == (uint8_t)whole, "the checksum's wire bytes");
	printf("file %08x %llu\n", fc.crc, (unsigned long long)fc.length);
	check(hdfs_crc_streams_combine(crcs, lens, NB, C, &combined) == 0 && combined == whole, "combine");
	check(hdfs_crc_streams_combine(crcs, lens, 0, C, &combined) == 0 && combined == 0, "combine of nothing");
	check(hdfs_crc_streams_combine(crcs, lens, NB, 0, &combined) == HDFS_CRC32C_EINVAL, "combine without a type");
	/* nothing of the caller's memory was written */
	check(hdfs_crc32c_memcpy(back, arena, arena_bytes, 1) == 0 && memcmp(back, host, arena_bytes) == 0,
	    "the arena is untouched");

	/* one seqno bit of entry 2's packet 3 flipped: that entry alone takes the other path, same CRC */
	{
		const uint64_t at = ((uint8_t *)e[2].stream - (uint8_t *)arena) + 3 * (31 + 32 + full) + 6 + 10;
		uint8_t bad = host[at] ^ 0x10;
		check(hdfs_crc32c_memcpy((uint8_t *)arena + at, &bad, 1, 0) == 0, "flip");
		check(hdfs_crc_streams_block_crcs(e, NB, V2, 512, C, NULL) == 0, "block_crcs");
		check(e[2].rc == 0 && e[2].path == HDFS_CRC_STREAMS_PATH_FALLBACK && e[2].nchunks == nchunks[2] &&
		    e[2].consumed == slen[2] && e[2].crc == want[2], "the flagged entry");
		check(e[0].path == HDFS_CRC_STREAMS_PATH_KERNEL && e[1].path == HDFS_CRC_STREAMS_PATH_KERNEL &&
		    e[0].crc == want[0] && e[1].crc == want[1], "the others");
		check(hdfs_crc32c_memcpy((uint8_t *)arena + at, host + at, 1, 0) == 0, "flip back");
	}

	/* refused, naming its entry: a host stream; and a stream from inside a block is no file's block */
	{
		const void *skeep = e[2].stream;
		e[2].stream = host;
		check(hdfs_crc_streams_block_crcs(e, NB, V2, 512, C, NULL) == HDFS_CRC32C_EINVAL &&
		    strstr(hdfs_crc_streams_last_error(), "entry 2"), "host stream refused");
		check(e[0].npkts == 0 && e[0].nchunks == 0 && e[0].crc == 0, "out fields zero after a refusal");
		e[2].stream = skeep;
		e[1].stream = (const uint8_t *)e[0].stream + 31 + 32 + full; /* entry 0 from its second packet on */
		e[1].len = slen[0] - (31 + 32 + full);
		check(hdfs_crc_streams_file_checksum(e, NB, V2, 512, C, NULL, &fc) == HDFS_CRC32C_EINVAL &&
		    strstr(hdfs_crc_streams_last_error(), "entry 1") && e[1].offset_in_block == (int64_t)full &&
		    e[1].rc == 0 && e[1].nchunks == nchunks[0] - 8, "a stream from inside a block");
	}

	/* the timing entry */
	{
		double ms = 0;
		check(hdfs_crc_streams_time(e, NB, V2, 512, C, HDFS_CRC_STREAMS_TIME_NONE, 2, &ms) == 0 && ms > 0 &&
		    e[2].crc == want[2], "timing entry");
		check(hdfs_crc_streams_time(e, NB, V2, 512, C, 1u, 2, &ms) == HDFS_CRC32C_EINVAL, "a flag bit refused");
	}

	free(host);
	free(back);
	hdfs_crc32c_dev_free(arena);
	printf("%d failures\n", failures);
	return failures != 0;
}
