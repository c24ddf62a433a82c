/*
 * C consumer of the relay batch library (include/hadoofus_relay_batch.h),
 * written the way a client that copies a file of several blocks from one
 * datanode to another would use it: three block transfers' packet streams (v2,
 * CRC32C; 5120-byte packets, a shorter one, the empty last one), built on the
 * host with a bitwise CRC of this file's own and uploaded at odd addresses of
 * one device allocation, are relayed by one call into the streams of three
 * writes.  Each output stream is sized by hdfs_relay_batch_layout and checked
 * by reading it back with hdfs_crc32c_read_packets: the payload, the writer's
 * offsets and sequence numbers, the last flag; one flipped data bit sends one
 * entry, and only that one, down the other path.
 * Prints "0 failures" on success.
 * Test infrastructure (tests/test_relay_batch_cpu.py links it on CPU,
 * tests/test_gpu_relay_batch.py runs it on the GPU).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_relay_batch.h"

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; relay batch: %s)\n", what, hdfs_crc32c_last_error(),
		    hdfs_relay_batch_last_error());
		failures++;
	}
}

static uint32_t crc32c_bitwise(const uint8_t *p, size_t n)
{
	uint32_t c = 0xFFFFFFFFu;
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

/* One v2 packet of dlen bytes of data at p; returns its end. */
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
		p = put_be(p, crc32c_bitwise(data + 512 * c, n), 4);
	}
	if (dlen)
		memcpy(p, data, dlen);
	return p + dlen;
}

#define NB 3
#define MAXP 8

int main(void)
{
	const uint32_t full = 5120, nfull[NB] = { 30, 1, 13 }, tail[NB] = { 700, 0, 513 };
	const int64_t woff[NB] = { 0, 3584, ((int64_t)1 << 31) + 512 }, wseq[NB] = { 0, 12345, 7 };
	const int V2 = HDFS_CRC32C_PROTO_V2, C = HDFS_CRC32C_CSUM_CRC32C;
	const size_t arena_bytes = 2 << 20, room = 170000;
	uint8_t *host = calloc(1, arena_bytes);
	void *arena = NULL;
	hdfs_relay_batch_entry e[NB];
	hdfs_crc32c_packet one[MAXP];
	uint64_t payload[NB], slen[NB], wlen[NB], wpk[NB];
	uint8_t *data[NB];

	check(hdfs_relay_batch_abi_version() == HDFS_RELAY_BATCH_ABI_VERSION, "abi version");
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0, "dev_alloc");
	memset(e, 0, sizeof(e));
	for (int b = 0; b < NB; b++) {
		uint8_t *s = host + 3 + b * 2 * room, *p = s;
		int64_t off = 1 << 20, seq = 0;
		payload[b] = (uint64_t)nfull[b] * full + tail[b];
		data[b] = malloc(payload[b]);
		for (uint64_t i = 0; i < payload[b]; i++)
			data[b][i] = (uint8_t)((i * 2654435761u + 97 * b) >> 7);
		for (uint32_t k = 0; k < nfull[b]; k++, off += full)
			p = put_packet(p, data[b] + (off - (1 << 20)), full, off, seq++, 0);
		if (tail[b])
			p = put_packet(p, data[b] + (off - (1 << 20)), tail[b], off, seq++, 0);
		p = put_packet(p, NULL, 0, off + tail[b], seq, 1);
		slen[b] = (uint64_t)(p - s);
		check(slen[b] < room, "a stream fits its room");
		check(hdfs_relay_batch_layout(payload[b], woff[b], V2, C, b != 1, &wlen[b], &wpk[b]) == 0 && wlen[b] < room,
		    "layout");
		e[b].stream = (uint8_t *)arena + (s - host);
		e[b].len = slen[b];
		e[b].offset_in_block = woff[b];
		e[b].seqno = wseq[b];
		e[b].finish = b != 1;
		e[b].wire = (uint8_t *)arena + (s - host) + room + 5;
		e[b].wire_cap = wlen[b];
	}
	check(hdfs_crc32c_memcpy(arena, host, arena_bytes, 0) == 0, "upload");

	/* the call */
	check(hdfs_relay_batch_relay(e, NB, V2, 512, C, NULL) == 0, "relay");
	for (int b = 0; b < NB; b++) {
		size_t n1 = 0;
		uint64_t used = 0, got = 0;
		hdfs_crc32c_iovec iov;
		uint8_t *back = malloc(payload[b]);
		check(e[b].rc == 0 && e[b].path == HDFS_RELAY_BATCH_PATH_KERNEL && e[b].consumed == slen[b] &&
		    e[b].delivered == payload[b] && e[b].src_offset_in_block == 1 << 20 && e[b].wire_len == wlen[b] &&
		    e[b].npkts == wpk[b], "an entry's outputs");
		/* the write's stream, read back: clean, the same payload, the writer's framing */
		iov.base = (uint8_t *)arena + 6 * room;
		iov.len = payload[b];
		check(hdfs_crc32c_read_packets(e[b].wire, e[b].wire_len, V2, 512, C, 0, HDFS_CRC32C_READ_ALL, &iov, 1, one,
		    MAXP, &n1, &used, &got) == 0 && n1 == wpk[b] && used == wlen[b] && got == payload[b],
		    "the output stream is clean");
		check(one[0].offset_in_block == woff[b] && one[0].seqno == wseq[b] &&
		    one[n1 - 1].seqno == wseq[b] + (int64_t)n1 - 1 && one[n1 - 1].last == (b != 1) &&
		    one[0].data_len == (int32_t)(payload[b] < 65536 ? payload[b] : 65536), "the writer's framing");
		check(hdfs_crc32c_memcpy(back, iov.base, payload[b], 1) == 0 && memcmp(back, data[b], payload[b]) == 0,
		    "an entry's payload");
		free(back);
	}
	printf("%llu + %llu + %llu bytes relayed\n", (unsigned long long)e[0].wire_len,
	    (unsigned long long)e[1].wire_len, (unsigned long long)e[2].wire_len);

	/* one data bit of entry 2's packet 3 flipped: that entry alone takes the other path */
	{
		const uint64_t at = ((uint8_t *)e[2].stream - (uint8_t *)arena) + 3 * (31 + 40 + full) + 31 + 40 + 1000;
		uint8_t bad = host[at] ^ 0x10;
		check(hdfs_crc32c_memcpy((uint8_t *)arena + at, &bad, 1, 0) == 0, "flip");
		check(hdfs_relay_batch_relay(e, NB, V2, 512, C, NULL) == HDFS_CRC32C_ERR_DATANODE_BAD_CHECKSUM,
		    "a bad checksum is the call's result");
		check(e[2].rc == HDFS_CRC32C_ERR_DATANODE_BAD_CHECKSUM && e[2].path == HDFS_RELAY_BATCH_PATH_FALLBACK &&
		    e[2].delivered == 3 * full && e[2].wire_len == 0 && e[2].npkts == 0, "the bad entry");
		check(e[0].rc == 0 && e[1].rc == 0 && e[0].path == HDFS_RELAY_BATCH_PATH_KERNEL &&
		    e[1].path == HDFS_RELAY_BATCH_PATH_KERNEL && e[0].wire_len == wlen[0], "the others");
		check(hdfs_crc32c_memcpy((uint8_t *)arena + at, host + at, 1, 0) == 0, "flip back");
	}

	/* a write off the chunk grid takes the other path and gives the same payload back */
	{
		uint64_t wl = 0, np = 0, used = 0, got = 0;
		size_t n1 = 0;
		hdfs_crc32c_iovec iov;
		e[1].offset_in_block = 4321;
		check(hdfs_relay_batch_layout(payload[1], 4321, V2, C, 0, &wl, &np) == 0 && np == 2 && wl <= room - 5, "layout");
		e[1].wire_cap = wl;
		check(hdfs_relay_batch_relay(e, NB, V2, 512, C, NULL) == 0 && e[1].path == HDFS_RELAY_BATCH_PATH_FALLBACK &&
		    e[1].wire_len == wl && e[1].npkts == np && e[2].path == HDFS_RELAY_BATCH_PATH_KERNEL, "unaligned write");
		iov.base = (uint8_t *)arena + 6 * room;
		iov.len = payload[1];
		check(hdfs_crc32c_read_packets(e[1].wire, wl, V2, 512, C, 0, HDFS_CRC32C_READ_ALL, &iov, 1, one, MAXP, &n1,
		    &used, &got) == 0 && n1 == 2 && got == payload[1] && one[0].offset_in_block == 4321 &&
		    one[0].data_len == 4608 - 4321, "the unaligned stream is clean");
		e[1].offset_in_block = woff[1];
		e[1].wire_cap = wlen[1];
	}

	/* refused, each naming its entry: a wire range over a stream, a host stream, a negative seqno */
	{
		void *keep = e[1].wire;
		e[1].wire = (uint8_t *)e[0].stream + 10;
		check(hdfs_relay_batch_relay(e, NB, V2, 512, C, NULL) == HDFS_CRC32C_EINVAL &&
		    strstr(hdfs_relay_batch_last_error(), "entry 1"), "overlap refused");
		e[1].wire = keep;
		const void *skeep = e[2].stream;
		e[2].stream = host;
		check(hdfs_relay_batch_relay(e, NB, V2, 512, C, NULL) == HDFS_CRC32C_EINVAL &&
		    strstr(hdfs_relay_batch_last_error(), "entry 2"), "host stream refused");
		e[2].stream = skeep;
		e[0].seqno = -1;
		check(hdfs_relay_batch_relay(e, NB, V2, 512, C, NULL) == HDFS_CRC32C_EINVAL &&
		    strstr(hdfs_relay_batch_last_error(), "entry 0"), "negative seqno refused");
		e[0].seqno = wseq[0];
	}

	/* the timing entry: two workgroups walk all packets */
	{
		double ms = 0;
		check(hdfs_relay_batch_time(e, NB, V2, 512, C, HDFS_RELAY_BATCH_TIME_GROUPS(2), 2, &ms) == 0 && ms > 0 &&
		    e[2].path == HDFS_RELAY_BATCH_PATH_KERNEL && e[2].wire_len == wlen[2], "timing entry");
		check(hdfs_relay_batch_time(e, NB, V2, 512, C, HDFS_RELAY_BATCH_TIME_GROUPS(1025), 2, &ms) ==
		    HDFS_CRC32C_EINVAL, "1025 workgroups refused");
	}

	for (int b = 0; b < NB; b++)
		free(data[b]);
	free(host);
	hdfs_crc32c_dev_free(arena);
	printf("%d failures\n", failures);
	return failures != 0;
}
