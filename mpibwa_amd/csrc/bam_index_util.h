// bam_index_util.h — what a BAI index (SAM specification §5.2) of a coordinate-sorted BAM file contains, stated once for the host path
// (bam_index.cpp), the device path (bam_index_kernel.hip, bam_sort_stage.hip), the stand-alone check (tests/csrc/bam_index_host_check.cpp)
// and, in words, tests/bam_index_model.py.  DESIGN §8.6.
//
// Per record (bam_util.h has the layout): refID, pos, l_read_name, n_cigar_op, flag and the CIGAR words are read, the stored bin is not.
//   refID = -1: counted in n_no_coor, nothing else.
//   refID >= 0: beg = max(pos, 0); rlen = the summed lengths of M, D, N, = and X, or 1 when flag 0x4 is set, n_cigar_op is 0 or the sum
//   is 0; end = beg + rlen; bin = reg2bin(beg, end); mapped = flag 0x4 clear.  end > 2^29 is beyond what BAI covers: the call fails.
//   CIGAR words that the record's own size does not hold are not read (the sort's validation does not look at them either).
// Virtual offsets, here in BLOCK-NUMBER space, block << 16 | offset in the block's payload: v0 of a record is that of its first byte
// (an empty block holds none), v1 is v0 of the next record, and of the last record (last non-empty block + 1) << 16.  Equal blocks are
// equal file offsets, so the join rule needs no file offsets; serialise() translates with the table of the blocks' file offsets.
// Bins: a maximal run of consecutive records of one contig and bin is a chunk [v0 of its first, v1 of its last); a bin's chunks stay in
// file order; a chunk that begins in the block in which its predecessor ends is joined to it, nothing else is (htslib's folding of
// small bins into their parents is not done); pseudo-bin 37450 behind the bins of a contig that has records.
// Linear index: n_intv = ((max end - 1) >> 14) + 1; ioffset[w] = v0 of the first record with beg < (w + 1) << 14 and end > w << 14; a
// window without one takes the nearest value before it, 0 when there is none.
#ifndef MBW_BAM_INDEX_UTIL_H
#define MBW_BAM_INDEX_UTIL_H
#include "bam_sort_util.h"
#include "bam_util.h"

namespace mbw {
namespace bidx {

constexpr uint64_t BAI_MAX_END = (uint64_t)1 << 29;
constexpr uint32_t BAI_PSEUDO_BIN = 37450;
constexpr uint64_t BAI_NO_RECORD = ~(uint64_t)0;      // a linear window that no record overlaps, before the fill
constexpr uint32_t BAI_REF_OPS = 0x18d;               // the CIGAR operations that cover reference bases: M 0, D 2, N 3, = 7, X 8
enum : int { BAI_OK = 0, BAI_BAD_BLOCK = 1, BAI_BAD_RECORD = 2, BAI_UNSORTED = 3, BAI_TOO_LONG = 4 };

struct Rec {
	int32_t ref;       // -1: no coordinate, the other fields are 0
	uint32_t beg;
	uint64_t end;      // beg + rlen; above BAI_MAX_END: the call fails
	uint32_t bin;
	uint32_t mapped;
};

// the well-formed record (bsort::record_at) of `size` bytes at s[at]
MBW_BS_HD Rec record_fields(const uint8_t *s, uint64_t at, uint32_t size)
{
	Rec r = {-1, 0, 0, 0, 0};
	const int32_t refid = (int32_t)bsort::load32(s, at + 4);
	if (refid < 0) return r;
	const int32_t pos = (int32_t)bsort::load32(s, at + 8);
	const uint32_t l_read_name = bsort::load32(s, at + 12) & 0xffu;
	const uint32_t w16 = bsort::load32(s, at + 16), n_cigar_op = w16 & 0xffffu, flag = w16 >> 16;
	const uint32_t cigar_at = 36 + l_read_name;
	uint32_t n = size > cigar_at ? (size - cigar_at) >> 2 : 0;
	if (n > n_cigar_op) n = n_cigar_op;
	uint64_t rlen = 0;
	for (uint32_t k = 0; k < n; ++k) {
		const uint32_t w = bsort::load32(s, at + cigar_at + 4ull * k);
		if ((BAI_REF_OPS >> (w & 15u)) & 1u) rlen += w >> 4;
	}
	if ((flag & 4u) || n_cigar_op == 0 || rlen == 0) rlen = 1;
	r.ref = refid;
	r.beg = pos > 0 ? (uint32_t)pos : 0;
	r.end = (uint64_t)r.beg + rlen;
	const uint64_t e = r.end > BAI_MAX_END ? BAI_MAX_END + 1 : r.end;   // (such a record fails the call: its bin is never written)
	r.bin = bam::reg2bin((int64_t)r.beg, (int64_t)e);
	r.mapped = (flag & 4u) ? 0u : 1u;
	return r;
}

// the block that holds byte p of the stream: cut[0 .. n_blk] are the blocks' first bytes and the stream's end, p < cut[n_blk]
MBW_BS_HD uint64_t block_of(const uint64_t *cut, uint64_t n_blk, uint64_t p)
{
	uint64_t lo = 0, hi = n_blk;   // the last b with cut[b] <= p: cut[b + 1] > p, so it is not empty
	while (hi - lo > 1) {
		const uint64_t mid = (lo + hi) >> 1;
		if (cut[mid] <= p) lo = mid; else hi = mid;
	}
	return lo;
}
MBW_BS_HD uint64_t voffset_of(const uint64_t *cut, uint64_t n_blk, uint64_t p)
{
	const uint64_t b = block_of(cut, n_blk, p);
	return b << 16 | (p - cut[b]);
}
// v1 of the file's last record
inline uint64_t end_voffset(const uint64_t *cut, uint64_t n_blk)
{
	uint64_t b = n_blk;
	while (b > 0 && cut[b] == cut[b - 1]) --b;
	return b << 16;
}

// the run's place in the order of the bins: the contig (n_ref: no coordinate) above the bin
MBW_BS_HD uint64_t run_key(int32_t ref, uint32_t bin, int32_t n_ref) { return (uint64_t)(uint32_t)(ref < 0 ? n_ref : ref) << 16 | bin; }
MBW_BS_HD uint32_t run_key_bits(int32_t n_ref) { return bsort::ref_bits(n_ref) + 16; }

// ---- host only: what either path hands to the serialiser ----
struct Parts {
	int32_t n_ref = 0;
	// the runs, sorted stably by run_key (runs without a coordinate, if any, stand last and are not written)
	std::vector<uint64_t> run_key, run_beg, run_end;
	// per contig: v0 of its first record, v1 of its last, mapped and unmapped records (both 0: none), the windows
	std::vector<uint64_t> stat;       // 4 * n_ref
	std::vector<uint32_t> n_intv;     // n_ref
	std::vector<uint64_t> ioffset;    // the contigs' windows back to back, BAI_NO_RECORD where no record overlaps
	uint64_t n_no_coor = 0;
	uint64_t n_chunks = 0;            // (out) chunks written, the pseudo-bins' not counted
};

inline void put32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
inline void put64(std::vector<uint8_t> &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k))); }

// the bytes of the index; blk_off[b]: the file offset of block b (one entry behind the last block: where the blocks end)
inline void serialise(Parts &P, const int64_t *blk_off, std::vector<uint8_t> &o)
{
	auto tr = [&](uint64_t v) { return (uint64_t)blk_off[v >> 16] << 16 | (v & 0xffffu); };
	o.clear();
	o.push_back('B'); o.push_back('A'); o.push_back('I'); o.push_back(1);
	put32(o, (uint32_t)P.n_ref);
	P.n_chunks = 0;
	size_t r = 0, w0 = 0;
	const size_t n_runs = P.run_key.size();
	std::vector<uint64_t> cb, ce;
	for (int32_t c = 0; c < P.n_ref; ++c) {
		const bool any = P.stat[4 * c + 2] + P.stat[4 * c + 3] != 0;
		const size_t n_bin_at = o.size();
		put32(o, 0);
		uint32_t n_bin = 0;
		while (r < n_runs && (P.run_key[r] >> 16) == (uint64_t)c) {
			const uint64_t key = P.run_key[r];
			cb.clear(); ce.clear();
			for (; r < n_runs && P.run_key[r] == key; ++r) {
				if (!cb.empty() && (P.run_beg[r] >> 16) == (ce.back() >> 16)) ce.back() = P.run_end[r];
				else { cb.push_back(P.run_beg[r]); ce.push_back(P.run_end[r]); }
			}
			put32(o, (uint32_t)(key & 0xffffu));
			put32(o, (uint32_t)cb.size());
			for (size_t k = 0; k < cb.size(); ++k) { put64(o, tr(cb[k])); put64(o, tr(ce[k])); }
			P.n_chunks += cb.size();
			++n_bin;
		}
		if (any) {
			put32(o, BAI_PSEUDO_BIN); put32(o, 2);
			put64(o, tr(P.stat[4 * c])); put64(o, tr(P.stat[4 * c + 1]));
			put64(o, P.stat[4 * c + 2]); put64(o, P.stat[4 * c + 3]);
			++n_bin;
		}
		for (int k = 0; k < 4; ++k) o[n_bin_at + k] = (uint8_t)(n_bin >> (8 * k));
		put32(o, P.n_intv[c]);
		uint64_t last = 0;
		for (uint32_t w = 0; w < P.n_intv[c]; ++w) {
			const uint64_t v = P.ioffset[w0 + w];
			if (v != BAI_NO_RECORD) last = tr(v);
			put64(o, last);
		}
		w0 += P.n_intv[c];
	}
	put64(o, P.n_no_coor);
}

} // namespace bidx
} // namespace mbw
#endif
