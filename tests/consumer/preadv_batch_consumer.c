/*
 * C consumer of the preadv batch library (include/hadoofus_preadv_batch.h),
 * written the way a client that reads many ranges straight into the places
 * they belong would use it: three reads' packet streams (v2, CRC32C; 4 KiB
 * packets, a shorter one, the empty last one; each stream starts at a chunk
 * boundary at or before the wanted offset), built on the host with a bitwise
 * CRC of this file's own and uploaded at odd addresses of one device
 * allocation, are served by one call, each into a list of device fragments
 * (rows of 100 bytes 128 bytes apart; one fragment; a one-byte fragment, an
 * empty one without a base and the rest).  The outputs are checked against
 * what the streams were built from and against hdfs_crc32c_read_packets of
 * each stream alone with a fragment list of the same lengths; one data bit
 * flipped in the skipped head of a packet 0 sends that entry, and only that
 * one, down the main library's path.
 * Prints "0 failures" on success.
 * Test infrastructure (tests/test_preadv_batch_cpu.py links it on CPU,
 * tests/test_gpu_preadv_batch.py runs it on the GPU).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_preadv_batch.h"

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; preadv batch: %s)\n", what, hdfs_crc32c_last_error(),
		    hdfs_preadv_batch_last_error());
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
#define MAXP 16
#define MAXF 256

/* The bytes the fragments hold, in order, out of a download of the arena. */
static int frags_equal(const uint8_t *back, const uint8_t *arena, const hdfs_crc32c_iovec *iov, int n,
    const uint8_t *want, uint64_t len)
{
	uint64_t at = 0;
	for (int i = 0; i < n && at < len; i++) {
		const uint64_t take = iov[i].len < len - at ? iov[i].len : len - at;
		if (take && memcmp(back + ((const uint8_t *)iov[i].base - arena), want + at, (size_t)take) != 0)
			return 0;
		at += take;
	}
	return at == len;
}

int main(void)
{
	const uint32_t full = 4096, nfull[NB] = { 5, 1, 9 }, tail[NB] = { 700, 0, 513 };
	/* the stream's first byte in the block, the read's first byte and its length */
	const int64_t block0[NB] = { 1 << 20, 0, 512 }, want0[NB] = { (1 << 20) + 300, 17, 512 + 4095 };
	const int64_t want[NB] = { 5 * 4096 + 650 - 300, 1, 3 * 4096 + 2 };
	const uint64_t npk[NB] = { 6, 1, 5 };   /* the packets each read takes */
	const int V2 = HDFS_CRC32C_PROTO_V2, C = HDFS_CRC32C_CSUM_CRC32C;
	const size_t arena_bytes = 1 << 20, room = 80000;
	uint8_t *host = calloc(1, arena_bytes), *back = malloc(arena_bytes);
	void *arena = NULL;
	hdfs_preadv_batch_entry e[NB];
	static hdfs_crc32c_iovec iov[NB][MAXF], alone[MAXF];
	int iovcnt[NB];
	hdfs_crc32c_packet pk[NB * MAXP], one[MAXP];
	uint64_t payload[NB], slen[NB];
	uint8_t *data[NB];

	check(hdfs_preadv_batch_abi_version() == HDFS_PREADV_BATCH_ABI_VERSION, "abi version");
	check(sizeof(hdfs_preadv_batch_entry) == 80, "the entry's size");
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0, "dev_alloc");
	memset(e, 0, sizeof(e));
	memset(host, 0xA5, arena_bytes);
	for (int b = 0; b < NB; b++) {
		uint8_t *s = host + 3 + b * 2 * room, *p = s;
		uint8_t *dst = (uint8_t *)arena + (s - host) + room + 5;
		int64_t off = 0, seq = 0;
		payload[b] = (uint64_t)nfull[b] * full + tail[b];
		data[b] = malloc(payload[b]);
		for (uint64_t i = 0; i < payload[b]; i++)
			data[b][i] = (uint8_t)((i * 2654435761u + 97 * b) >> 7);
		for (uint32_t k = 0; k < nfull[b]; k++, off += full)
			p = put_packet(p, data[b] + off, full, block0[b] + off, seq++, 0);
		if (tail[b])
			p = put_packet(p, data[b] + off, tail[b], block0[b] + off, seq++, 0);
		p = put_packet(p, NULL, 0, block0[b] + (int64_t)payload[b], seq, 1);
		slen[b] = (uint64_t)(p - s);
		e[b].stream = (uint8_t *)arena + (s - host);
		e[b].len = slen[b];
		e[b].client_offset = want0[b];
		e[b].read_len = want[b];
		if (b == 0) {           /* rows of 100 bytes, 128 bytes apart */
			iovcnt[b] = (int)((want[b] + 99) / 100);
			for (int i = 0; i < iovcnt[b]; i++) {
				iov[b][i].base = dst + 128 * i;
				iov[b][i].len = 100;
			}
		} else if (b == 1) {    /* one fragment with room behind the read */
			iovcnt[b] = 1;
			iov[b][0].base = dst;
			iov[b][0].len = (uint64_t)want[b] + 9;
		} else {                /* one byte, an empty fragment without a base, the rest */
			iovcnt[b] = 3;
			iov[b][0].base = dst;
			iov[b][0].len = 1;
			iov[b][1].base = NULL;
			iov[b][1].len = 0;
			iov[b][2].base = dst + 40;
			iov[b][2].len = (uint64_t)want[b] - 1;
		}
		e[b].iov = iov[b];
		e[b].iovcnt = iovcnt[b];
	}
	check(hdfs_crc32c_memcpy(arena, host, arena_bytes, 0) == 0, "upload");

	/* the call */
	check(hdfs_preadv_batch_read(e, NB, V2, 512, C, pk, MAXP, NULL) == 0, "read");
	check(hdfs_crc32c_memcpy(back, arena, arena_bytes, 1) == 0, "download");
	for (int b = 0; b < NB; b++) {
		const int64_t c_begin = want0[b] - block0[b];
		const uint8_t *first = back + ((uint8_t *)iov[b][0].base - (uint8_t *)arena);
		check(e[b].rc == 0 && e[b].path == HDFS_PREADV_BATCH_PATH_KERNEL && e[b].npkts == npk[b] &&
		    e[b].delivered == (uint64_t)want[b] && e[b].consumed < slen[b], "an entry's outputs");
		check(pk[b * MAXP].seqno == 0 && pk[b * MAXP].offset_in_block == block0[b] &&
		    pk[b * MAXP + npk[b] - 1].seqno == (int64_t)npk[b] - 1 && pk[b * MAXP + npk[b] - 1].data_len != 0,
		    "an entry's records");
		check(frags_equal(back, arena, iov[b], iovcnt[b], data[b] + c_begin, (uint64_t)want[b]), "an entry's bytes");
		check(first[-1] == 0xA5 && first[iov[b][0].len] == 0xA5, "nothing around the first fragment");
		/* and what the main library says of the stream and window alone, into fragments of the same lengths */
		size_t n1 = 0;
		uint64_t used = 0, gotn = 0, at = 0;
		for (int i = 0; i < iovcnt[b]; i++) {
			alone[i].base = iov[b][i].len ? (uint8_t *)arena + 900000 + at : NULL;
			alone[i].len = iov[b][i].len;
			at += iov[b][i].len;
		}
		check(hdfs_crc32c_read_packets(e[b].stream, e[b].len, V2, 512, C, want0[b], want[b], alone, iovcnt[b], one,
		    MAXP, &n1, &used, &gotn) == 0 && n1 == e[b].npkts && used == e[b].consumed && gotn == e[b].delivered &&
		    memcmp(one, pk + b * MAXP, n1 * sizeof(one[0])) == 0, "read_packets of the stream alone");
	}
	check(back[((uint8_t *)iov[0][0].base - (uint8_t *)arena) + 100] == 0xA5, "the gap between two rows");
	printf("%llu + %llu + %llu bytes delivered\n", (unsigned long long)e[0].delivered,
	    (unsigned long long)e[1].delivered, (unsigned long long)e[2].delivered);

	/* one data bit in the skipped head of entry 0's packet 0 flipped: that entry alone takes the other path */
	{
		const uint64_t at = ((uint8_t *)e[0].stream - (uint8_t *)arena) + 31 + 32 + 100;
		uint8_t bad = host[at] ^ 0x10;
		check(hdfs_crc32c_memcpy((uint8_t *)arena + at, &bad, 1, 0) == 0, "flip");
		check(hdfs_preadv_batch_read(e, NB, V2, 512, C, pk, MAXP, NULL) == HDFS_CRC32C_ERR_DATANODE_BAD_CHECKSUM,
		    "a bad checksum is the call's result");
		check(e[0].rc == HDFS_CRC32C_ERR_DATANODE_BAD_CHECKSUM && e[0].path == HDFS_PREADV_BATCH_PATH_FALLBACK &&
		    e[0].delivered == 0 && e[0].npkts == 1 && pk[0].first_bad == 0 && pk[0].bad_chunks == 1, "the bad entry");
		check(e[1].rc == 0 && e[2].rc == 0 && e[1].path == HDFS_PREADV_BATCH_PATH_KERNEL &&
		    e[2].path == HDFS_PREADV_BATCH_PATH_KERNEL, "the others");
		check(hdfs_crc32c_memcpy((uint8_t *)arena + at, host + at, 1, 0) == 0, "flip back");
	}

	/* fragments three bytes short of the read: AGAIN, resumed by a second call into a last fragment */
	{
		hdfs_preadv_batch_entry r = e[2], r2 = e[2];
		hdfs_crc32c_iovec shorter[3], rest;
		memcpy(shorter, iov[2], sizeof(shorter));
		shorter[2].len -= 3;
		r.iov = shorter;
		check(hdfs_preadv_batch_read(&r, 1, V2, 512, C, NULL, 0, NULL) == HDFS_CRC32C_AGAIN &&
		    r.rc == HDFS_CRC32C_AGAIN && r.delivered == (uint64_t)want[2] - 3 &&
		    r.path == HDFS_PREADV_BATCH_PATH_FALLBACK, "AGAIN");
		rest.base = (uint8_t *)iov[2][2].base + shorter[2].len;
		rest.len = 3;
		r2.stream = (const uint8_t *)e[2].stream + r.consumed;
		r2.len = e[2].len - r.consumed;
		r2.iov = &rest;
		r2.iovcnt = 1;
		r2.client_offset = want0[2] + (int64_t)r.delivered;
		r2.read_len = 3;
		check(hdfs_preadv_batch_read(&r2, 1, V2, 512, C, NULL, 0, NULL) == 0 && r2.delivered == 3 &&
		    r2.path == HDFS_PREADV_BATCH_PATH_KERNEL, "the resumed read");
		check(hdfs_crc32c_memcpy(back, arena, arena_bytes, 1) == 0, "download");
		check(frags_equal(back, arena, iov[2], 3, data[2] + 4095, (uint64_t)want[2]), "the joined bytes");
	}

	/* refused, each naming its entry and fragment: a fragment over a stream, a host fragment, no fragments */
	{
		void *keep = iov[1][0].base;
		iov[1][0].base = (uint8_t *)e[0].stream + 10;
		check(hdfs_preadv_batch_read(e, NB, V2, 512, C, pk, MAXP, NULL) == HDFS_CRC32C_EINVAL &&
		    strstr(hdfs_preadv_batch_last_error(), "entry 1") && strstr(hdfs_preadv_batch_last_error(), "fragment 0"),
		    "overlap refused");
		iov[1][0].base = keep;
		keep = iov[2][2].base;
		iov[2][2].base = host;
		check(hdfs_preadv_batch_read(e, NB, V2, 512, C, pk, MAXP, NULL) == HDFS_CRC32C_EINVAL &&
		    strstr(hdfs_preadv_batch_last_error(), "entry 2") && strstr(hdfs_preadv_batch_last_error(), "fragment 2"),
		    "host fragment refused");
		iov[2][2].base = keep;
		e[0].iovcnt = 0;
		check(hdfs_preadv_batch_read(e, NB, V2, 512, C, pk, MAXP, NULL) == HDFS_CRC32C_EINVAL &&
		    strstr(hdfs_preadv_batch_last_error(), "entry 0"), "iovcnt 0 refused");
		e[0].iovcnt = iovcnt[0];
	}

	/* the timing entry: two workgroups walk all packets */
	{
		double ms = 0;
		check(hdfs_preadv_batch_time(e, NB, V2, 512, C, HDFS_PREADV_BATCH_TIME_GROUPS(2), 2, &ms) == 0 && ms > 0 &&
		    e[0].path == HDFS_PREADV_BATCH_PATH_KERNEL && e[0].delivered == (uint64_t)want[0], "timing entry");
		check(hdfs_preadv_batch_time(e, NB, V2, 512, C, HDFS_PREADV_BATCH_TIME_GROUPS(1025), 2, &ms) ==
		    HDFS_CRC32C_EINVAL, "1025 workgroups refused");
	}

	for (int b = 0; b < NB; b++)
		free(data[b]);
	free(host);
	free(back);
	hdfs_crc32c_dev_free(arena);
	printf("%d failures\n", failures);
	return failures != 0;
}
