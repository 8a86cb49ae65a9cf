// bam_sort_host_check.cpp — csrc/bam_sort_util.h on the host, in a program of its own (tests/test_bam_sort_util_host.py builds it with
// the address and undefined-behaviour sanitizers where the compiler has them): the header, the hop, the validation and the key over
// inflated BAM streams that are held in heap blocks of their exact sizes, so that a read past a stream's end is a sanitizer report.
//
//     bam_sort_host_check FILE        FILE: entries of uint32 size | the stream
// prints one line per entry:  code n_ref h_end n_records fnv(offset, size, key of every record) fnv(the rewritten header)
// code: 0, or -(offset) - 1 of what parse_header or record_at refuses (a header that the stream cuts off: the stream's size).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bam_sort_util.h"

using namespace mbw;

static uint32_t fnv(uint32_t h, const void *p, size_t n)
{
	const uint8_t *b = (const uint8_t *)p;
	for (size_t k = 0; k < n; ++k) h = (h ^ b[k]) * 16777619u;
	return h;
}

int main(int argc, char **argv)
{
	if (argc != 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	uint32_t size;
	while (fread(&size, 4, 1, f) == 1) {
		uint8_t *s = (uint8_t *)malloc(size ? size : 1);   // the exact size: nothing behind the stream belongs to it
		if (size && fread(s, 1, size, f) != size) return 2;
		bsort::Header h;
		int64_t code = bsort::parse_header(s, size, h);
		uint32_t hash = 2166136261u, hhash = 2166136261u;
		uint64_t n_rec = 0;
		if (code > 0) code = -(int64_t)size - 1;
		if (code == 0) {
			std::vector<uint8_t> head;
			bsort::coordinate_header(s, h, head);
			hhash = fnv(hhash, head.data(), head.size());
			for (uint64_t at = h.end; at < size;) {
				uint32_t sz;
				uint64_t key;
				if (!bsort::record_at(s, at, size, h.n_ref, &sz, &key)) { code = -(int64_t)at - 1; break; }
				hash = fnv(hash, &at, 8); hash = fnv(hash, &sz, 4); hash = fnv(hash, &key, 8);
				if (key >> bsort::key_bits(h.n_ref)) return 3;   // a key outside the bits the sort runs over
				at += sz; ++n_rec;
			}
		}
		printf("%" PRId64 " %d %" PRIu64 " %" PRIu64 " %08x %08x\n", code, h.n_ref, h.end, n_rec, hash, hhash);
		free(s);
	}
	fclose(f);
	return 0;
}
