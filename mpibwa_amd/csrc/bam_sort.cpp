// bam_sort.cpp — mi355x_bam_sort: a finished BAM file to coordinate order on the rank's host threads, and what the device path
// (bam_sort_stage.hip) shares with it: the bound, the record walk, the header's blocks and the cuts.  DESIGN §8.5.  Host code, no GPU.
//
// The file's blocks are inflated side by side (mi355x_bgzf_inflate), the header is parsed and its @HD line rewritten, one hop from
// record to record gives offsets, sizes and keys (bam_sort_util.h), a stable sort of (key, index) orders them, the records are copied
// into that order and cut into blocks of whole records (bam_cuts), and the blocks are compressed side by side by zlib.  The header's
// blocks, the records' blocks and the empty end block follow each other in the output.
//
// Error offsets: a bad BGZF block (a header that is none, a block that the file cuts off, a failed inflate, CRC or ISIZE) is reported by
// its offset in the INPUT FILE, as mi355x_bgzf_inflate reports it; a bad BAM header or record by its offset in the INFLATED STREAM.  The
// blocks are checked first, so a file with both gives the block's.
#include "internal.h"
#include "bam_sort_util.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>

using namespace mbw;

namespace mbw {

constexpr size_t BS_BLOCK = 0xff00, BS_SLOT = 0x10000;

int64_t bam_sort_walk(const uint8_t *s, uint64_t h_end, uint64_t u, int32_t n_ref, std::vector<uint64_t> &off, std::vector<uint32_t> &size,
                      std::vector<uint64_t> &key)
{
	off.clear(); size.clear(); key.clear();
	for (uint64_t at = h_end; at < u;) {
		uint32_t sz;
		uint64_t k;
		if (!bsort::record_at(s, at, u, n_ref, &sz, &k)) return -(int64_t)at - 1;
		off.push_back(at); size.push_back(sz); key.push_back(k);
		at += sz;
	}
	return 0;
}

// Room for the sorted file of an inflated stream of u bytes.  A block holds at most BS_BLOCK bytes and is at most 31 bytes larger than
// its payload when zlib or the device deflate stores it (18 + 8 of BGZF, 5 of one stored deflate block).  Blocks, with R bytes of
// records and H of header, R + H = bytes: two neighbours of whole records hold more than BS_BLOCK bytes together, a record above
// BS_BLOCK bytes gives at most size / BS_BLOCK + 1 blocks and may stand behind a lone small block, so the records have fewer than
// 3 R / BS_BLOCK + 2 blocks; the header has fewer than H / BS_BLOCK + 1.  Together fewer than 3 bytes / BS_BLOCK + 3, which
// 3 * (bytes / BS_BLOCK + 1) + 3 covers whatever the division drops.
uint64_t bam_sort_bound_of(uint64_t u)
{
	const uint64_t bytes = u + bsort::BAM_SORT_HEADER_GROWTH;
	return bytes + 31 * (3 * (bytes / BS_BLOCK + 1) + 3) + 28;
}

// the cuts of the output stream: the new header of hn bytes in blocks of its own, then the records' blocks (rec_off[0 .. n] from 0)
void bam_sort_cuts(uint64_t hn, const std::vector<uint64_t> &rec_off, std::vector<size_t> &cut)
{
	std::vector<size_t> rc;
	bam_cuts(rec_off, rc);
	cut.assign(1, 0);
	for (uint64_t at = 0; at < hn;) {
		at = std::min<uint64_t>(hn, at + BS_BLOCK);
		cut.push_back((size_t)at);
	}
	for (size_t k = 1; k < rc.size(); ++k) cut.push_back((size_t)hn + rc[k]);
}

} // namespace mbw

extern "C" int64_t mi355x_bam_sort_bound(const uint8_t *bam, size_t len)
{
	std::vector<int64_t> blk, txt;
	const int64_t bad = bgzf_in_plan(bam, len, blk, txt);
	if (bad >= 0) return -bad - 1;
	return (int64_t)bam_sort_bound_of((uint64_t)txt.back());
}

extern "C" int64_t mi355x_bam_sort(const uint8_t *bam, size_t len, int level, uint8_t *out, size_t cap)
{
	if (level > 9 || level < 0) level = -1;   // zlib's default
	std::vector<int64_t> blk, txt;
	const int64_t bad = bgzf_in_plan(bam, len, blk, txt);
	const uint64_t u = (uint64_t)txt.back();
	std::vector<uint8_t> text((size_t)u + 1);
	const int64_t r = mi355x_bgzf_inflate(bam, len, (char *)text.data(), (size_t)u + 1);
	if (r < 0) return r;
	if (bad >= 0) return -bad - 1;
	bsort::Header h;
	const int64_t hs = bsort::parse_header(text.data(), u, h);
	if (hs < 0) return hs;
	if (hs > 0) return -(int64_t)u - 1;   // the stream ends inside the header
	std::vector<uint64_t> off, key;
	std::vector<uint32_t> size;
	const int64_t ws = bam_sort_walk(text.data(), h.end, u, h.n_ref, off, size, key);
	if (ws < 0) return ws;
	if ((uint64_t)cap < bam_sort_bound_of(u)) return 0;
	const size_t n = off.size();
	if (n > 0xffffffffull) die("mi355x_bam_sort: %zu records", n);

	// the order: (key, index) sorted stably by key — chunks side by side, then merged pair by pair
	std::vector<std::pair<uint64_t, uint32_t>> ord(n);
	for (size_t i = 0; i < n; ++i) ord[i] = {key[i], (uint32_t)i};
	std::vector<uint64_t>().swap(key);
	auto less = [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) { return a.first < b.first; };
	const size_t n_chunks = n >= (1u << 16) ? 64 : 1;
	auto edge = [&](size_t c) { return n / n_chunks * c + std::min(c, n % n_chunks); };
	host_parallel((int64_t)n_chunks, 1, [&](int64_t lo, int64_t hi) {
		for (int64_t c = lo; c < hi; ++c) std::stable_sort(ord.begin() + edge(c), ord.begin() + edge(c + 1), less);
	});
	for (size_t w = 1; w < n_chunks; w *= 2)
		host_parallel((int64_t)(n_chunks / (2 * w)), 1, [&](int64_t lo, int64_t hi) {
			for (int64_t p = lo; p < hi; ++p)
				std::inplace_merge(ord.begin() + edge(2 * w * p), ord.begin() + edge(2 * w * p + w), ord.begin() + edge(2 * w * p + 2 * w), less);
		});

	// the output stream: the new header, then the records in their order
	std::vector<uint8_t> head;
	bsort::coordinate_header(text.data(), h, head);
	std::vector<uint64_t> rec_off(n + 1);
	rec_off[0] = 0;
	for (size_t i = 0; i < n; ++i) rec_off[i + 1] = rec_off[i] + size[ord[i].second];
	std::vector<uint8_t> stream(head.size() + (size_t)rec_off[n]);
	memcpy(stream.data(), head.data(), head.size());
	host_parallel((int64_t)n, 4096, [&](int64_t lo, int64_t hi) {
		for (int64_t i = lo; i < hi; ++i) memcpy(stream.data() + head.size() + rec_off[i], text.data() + off[ord[i].second], size[ord[i].second]);
	});
	std::vector<uint8_t>().swap(text);
	std::vector<size_t> cut;
	bam_sort_cuts(head.size(), rec_off, cut);
	// every block into a slot of its own, closed up; then the whole into out (the slots' pages are touched only as far as the blocks reach)
	uint8_t *slots = (uint8_t *)malloc((cut.size() - 1) * BS_SLOT + 1);
	if (!slots) die("mi355x_bam_sort: out of memory");
	const size_t w = bgzf_blocks_at(stream.data(), cut, level, slots);
	if (w + 28 > cap) die("mi355x_bam_sort: %zu bytes of blocks above the bound %zu", w + 28, (size_t)bam_sort_bound_of(u));
	memcpy(out, slots, w);
	free(slots);
	return (int64_t)(w + mi355x_bgzf_eof(out + w));
}
