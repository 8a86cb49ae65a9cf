// bam_index_host_check.cpp — csrc/bam_index_util.h on the host, in a program of its own (tests/test_bam_index_util_host.py builds it
// with the address and undefined-behaviour sanitizers where the compiler has them): every record's contig, interval, bin and mapped bit,
// and its virtual offset under cuts every 1000 bytes with an empty block behind the first, over inflated BAM streams that are held in
// heap blocks of their exact sizes, so that a read past a stream's end is a sanitizer report.
//
//     bam_index_host_check FILE        FILE: entries of uint32 size | the stream
// prints one line per entry:  code n_records n_too_long fnv(offset, ref, beg, end, bin, mapped, v0 of every record)
// code: 0, or -(offset) - 1 of what parse_header or record_at refuses (a header that the stream cuts off: the stream's size).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bam_index_util.h"

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
		std::vector<uint64_t> cut = {0};
		for (uint64_t at = 0; at < size;) {
			at = at + 1000 < size ? at + 1000 : size;
			cut.push_back(at);
			if (cut.size() == 2) cut.push_back(at);   // block 1 is empty
		}
		const uint64_t n_blk = cut.size() - 1;
		bsort::Header h;
		int64_t code = bsort::parse_header(s, size, h);
		uint32_t hash = 2166136261u;
		uint64_t n_rec = 0, n_long = 0;
		if (code > 0) code = -(int64_t)size - 1;
		if (code == 0) {
			for (uint64_t at = h.end; at < size;) {
				uint32_t sz;
				uint64_t key;
				if (!bsort::record_at(s, at, size, h.n_ref, &sz, &key)) { code = -(int64_t)at - 1; break; }
				const bidx::Rec r = bidx::record_fields(s, at, sz);
				const uint64_t v0 = bidx::voffset_of(cut.data(), n_blk, at);
				const int64_t ref = r.ref;
				const uint64_t beg = r.beg, bin = r.bin, mapped = r.mapped;
				hash = fnv(hash, &at, 8); hash = fnv(hash, &ref, 8); hash = fnv(hash, &beg, 8); hash = fnv(hash, &r.end, 8);
				hash = fnv(hash, &bin, 8); hash = fnv(hash, &mapped, 8); hash = fnv(hash, &v0, 8);
				if (r.end > bidx::BAI_MAX_END) ++n_long;
				if (bidx::run_key(r.ref, r.bin, h.n_ref) >> bidx::run_key_bits(h.n_ref)) return 3;   // a key outside the bits the runs' sort runs over
				at += sz; ++n_rec;
			}
			if (bidx::end_voffset(cut.data(), n_blk) != (n_blk == 2 ? 1u : n_blk) << 16) return 4;
		}
		printf("%" PRId64 " %" PRIu64 " %" PRIu64 " %08x\n", code, n_rec, n_long, hash);
		free(s);
	}
	fclose(f);
	return 0;
}
