// bam_index.cpp — mi355x_bam_index: the BAI index of a coordinate-sorted BAM file in memory, on the rank's host threads.  DESIGN §8.6.
// Host code, no GPU.  The rules are bam_index_util.h's; the device path (bam_sort_stage.hip) comes here for a file it leaves to the host.
//
// The file's blocks are inflated side by side (mi355x_bgzf_inflate), the header is parsed, one hop from record to record checks the
// order and takes every record's contig, interval, bin and virtual offset; the runs of one bin are sorted stably by (contig, bin), the
// linear windows take the first record that reaches them, and bidx::serialise writes the bytes.
//
// Error offsets as in bam_sort.cpp: a bad BGZF block by its offset in the INPUT FILE, and first; a bad header or record, a record that
// sorts before its predecessor and a record that ends beyond 2^29 by its offset in the INFLATED STREAM, the first such record in stream
// order.
#include "internal.h"
#include "bam_index_util.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

using namespace mbw;

namespace mbw {

// the index of the inflated stream s[0 .. u) whose blocks are blk / txt (bgzf_in_plan's tables); the number of records, or
// -(offset) - 1 and the reason
int64_t bam_index_stream(const uint8_t *s, uint64_t u, const std::vector<int64_t> &blk, const std::vector<int64_t> &txt, std::vector<uint8_t> &bai, int *reason)
{
	bsort::Header h;
	const int64_t hs = bsort::parse_header(s, u, h);
	*reason = bidx::BAI_BAD_RECORD;
	if (hs < 0) return hs;
	if (hs > 0) return -(int64_t)u - 1;   // the stream ends inside the header
	const uint64_t n_blk = blk.size() - 1;
	std::vector<uint64_t> cut(txt.begin(), txt.end());
	const uint64_t end_v = bidx::end_voffset(cut.data(), n_blk);

	bidx::Parts P;
	P.n_ref = h.n_ref;
	P.stat.assign(4 * (size_t)h.n_ref, 0);
	std::vector<uint64_t> max_end((size_t)h.n_ref, 0);
	std::vector<std::vector<uint64_t>> lin((size_t)h.n_ref);
	std::vector<uint64_t> rk, rb, re;   // the runs in file order
	uint64_t prev_key = 0, n_rec = 0, b = 0;
	int32_t last_ref = -1;
	for (uint64_t at = h.end; at < u; ++n_rec) {
		uint32_t size;
		uint64_t key;
		if (!bsort::record_at(s, at, u, h.n_ref, &size, &key)) return -(int64_t)at - 1;
		if (key < prev_key) { *reason = bidx::BAI_UNSORTED; return -(int64_t)at - 1; }
		prev_key = key;
		const bidx::Rec r = bidx::record_fields(s, at, size);
		if (r.end > bidx::BAI_MAX_END) { *reason = bidx::BAI_TOO_LONG; return -(int64_t)at - 1; }
		while (cut[b + 1] <= at) ++b;   // (at < u = cut[n_blk])
		const uint64_t v0 = b << 16 | (at - cut[b]);
		if (!re.empty()) re.back() = v0;
		if (last_ref >= 0) P.stat[4 * (size_t)last_ref + 1] = v0;
		const uint64_t k = bidx::run_key(r.ref, r.bin, h.n_ref);
		if (rk.empty() || rk.back() != k) { rk.push_back(k); rb.push_back(v0); re.push_back(v0); }
		last_ref = r.ref;
		if (r.ref < 0) { P.n_no_coor += 1; at += size; continue; }
		const size_t c = (size_t)r.ref;
		if (P.stat[4 * c + 2] + P.stat[4 * c + 3] == 0) P.stat[4 * c] = v0;
		P.stat[4 * c + (r.mapped ? 2 : 3)] += 1;
		if (r.end > max_end[c]) {
			max_end[c] = r.end;
			lin[c].resize((size_t)((r.end - 1) >> 14) + 1, bidx::BAI_NO_RECORD);
		}
		for (uint64_t w = r.beg >> 14; w <= (r.end - 1) >> 14; ++w)
			if (lin[c][w] == bidx::BAI_NO_RECORD) lin[c][w] = v0;
		at += size;
	}
	if (!re.empty()) re.back() = end_v;
	if (last_ref >= 0) P.stat[4 * (size_t)last_ref + 1] = end_v;

	std::vector<uint32_t> ord(rk.size());
	std::iota(ord.begin(), ord.end(), 0u);
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t c) { return rk[a] < rk[c]; });
	P.run_key.resize(rk.size()); P.run_beg.resize(rk.size()); P.run_end.resize(rk.size());
	for (size_t q = 0; q < ord.size(); ++q) { P.run_key[q] = rk[ord[q]]; P.run_beg[q] = rb[ord[q]]; P.run_end[q] = re[ord[q]]; }
	P.n_intv.resize((size_t)h.n_ref);
	for (size_t c = 0; c < (size_t)h.n_ref; ++c) {
		P.n_intv[c] = (uint32_t)lin[c].size();
		P.ioffset.insert(P.ioffset.end(), lin[c].begin(), lin[c].end());
	}
	bidx::serialise(P, blk.data(), bai);
	*reason = bidx::BAI_OK;
	return (int64_t)n_rec;
}

// malloc'ed bytes for the caller (free), as mi355x_route_by_chr hands its outputs over
void bam_index_hand_over(const std::vector<uint8_t> &bai, uint8_t **out, size_t *out_len)
{
	uint8_t *p = (uint8_t *)malloc(bai.size() ? bai.size() : 1);
	if (!p) die("mi355x_bam_index: out of memory");
	memcpy(p, bai.data(), bai.size());
	*out = p;
	*out_len = bai.size();
}

int64_t bam_index_host(const uint8_t *bam, size_t len, std::vector<uint8_t> &bai, int *reason)
{
	std::vector<int64_t> blk, txt;
	const int64_t bad = bgzf_in_plan(bam, len, blk, txt);
	const uint64_t u = (uint64_t)txt.back();
	std::vector<uint8_t> text((size_t)u + 1);
	const int64_t r = mi355x_bgzf_inflate(bam, len, (char *)text.data(), (size_t)u + 1);
	*reason = bidx::BAI_BAD_BLOCK;
	if (r < 0) return r;
	if (bad >= 0) return -bad - 1;
	return bam_index_stream(text.data(), u, blk, txt, bai, reason);
}

} // namespace mbw

extern "C" int64_t mi355x_bam_index(const uint8_t *bam, size_t len, uint8_t **bai, size_t *bai_len, int *reason)
{
	std::vector<uint8_t> bytes;
	int why = 0;
	const int64_t n = bam_index_host(bam, len, bytes, &why);
	if (reason) *reason = why;
	if (n >= 0) bam_index_hand_over(bytes, bai, bai_len);
	return n;
}
