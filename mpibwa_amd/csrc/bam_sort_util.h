// bam_sort_util.h — the coordinate order of BAM records, stated once for the host path (bam_sort.cpp), the device path
// (bam_sort_kernel.hip, bam_sort_stage.hip) and the stand-alone check (tests/csrc/bam_sort_host_check.cpp): the hop from a record to the
// next, what makes a record malformed, the sort key and its packing, and the header's @HD line.  DESIGN §8.5.
//
// A record starts with int32 block_size (little-endian, at any byte alignment); the next record starts 4 + block_size further on.  Of
// the 32 fixed bytes behind block_size the order reads refID (+4), pos (+8) and flag (+18), nothing else (bam_util.h has the layout).
//
// No function here reads a byte at or beyond the `end` it is given, on the host.  The device build reads whole aligned dwords, at most
// 7 bytes beyond a field: the stream's buffer has BAM_SORT_SLACK bytes behind its end for that.
#ifndef MBW_BAM_SORT_UTIL_H
#define MBW_BAM_SORT_UTIL_H
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define MBW_BS_HD __host__ __device__ inline
#else
#define MBW_BS_HD inline
#endif

namespace mbw {
namespace bsort {

constexpr uint32_t BAM_SORT_SLACK = 64;     // bytes a device buffer of the stream has behind its end
constexpr uint32_t BAM_MIN_BLOCK_SIZE = 32; // the fixed fields behind block_size

// the 32-bit little-endian word at s[at], at any alignment
MBW_BS_HD uint32_t load32(const uint8_t *s, uint64_t at)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const uint64_t a = at & ~(uint64_t)3;
	const uint32_t *w = (const uint32_t *)(s + a);   // (s is a device allocation's start: aligned)
	const uint32_t sh = (uint32_t)(at & 3u);
	const uint32_t lo = w[0];
	if (!sh) return lo;
	return __builtin_amdgcn_alignbyte(w[1], lo, sh);
#else
	return (uint32_t)s[at] | (uint32_t)s[at + 1] << 8 | (uint32_t)s[at + 2] << 16 | (uint32_t)s[at + 3] << 24;
#endif
}

// bits of the key that hold the contig: the values 0 .. n_ref (n_ref: no contig) need ceil(log2(n_ref + 1)) of them
MBW_BS_HD uint32_t ref_bits(int32_t n_ref)
{
	uint32_t b = 0;
	while (((uint64_t)1 << b) < (uint64_t)n_ref + 1) ++b;
	return b;
}
// bits of the whole key: the radix sort runs over these only
MBW_BS_HD uint32_t key_bits(int32_t n_ref) { return ref_bits(n_ref) + 32 + 1; }

// samtools' coordinate order in one word: the contig (refID -1 behind every contig), pos + 1, the reverse-strand bit
MBW_BS_HD uint64_t pack_key(int32_t refid, int32_t pos, uint32_t flag, int32_t n_ref)
{
	const uint64_t ref = refid < 0 ? (uint64_t)(uint32_t)n_ref : (uint64_t)(uint32_t)refid;
	return ref << 33 | (uint64_t)(uint32_t)(pos + 1) << 1 | (uint64_t)((flag >> 4) & 1u);
}

// The record at s[at] of a stream (or a part of one) that ends at `end`, at < end.  true: well-formed; *size = 4 + block_size, the hop;
// *key = its packed key.  false: malformed — block_size < 32, a record that runs past end (a block_size that does not fit before end
// included), refID < -1 or >= n_ref, pos < -1.
MBW_BS_HD bool record_at(const uint8_t *s, uint64_t at, uint64_t end, int32_t n_ref, uint32_t *size, uint64_t *key)
{
	if (end - at < 4) return false;
	const uint32_t block_size = load32(s, at);
	if (block_size < BAM_MIN_BLOCK_SIZE || block_size > 0x7fffffffu) return false;
	if ((uint64_t)block_size + 4 > end - at) return false;
	const int32_t refid = (int32_t)load32(s, at + 4), pos = (int32_t)load32(s, at + 8);
	if (refid < -1 || refid >= n_ref || pos < -1) return false;
	const uint32_t flag = load32(s, at + 16) >> 16;
	*size = block_size + 4;
	*key = pack_key(refid, pos, flag, n_ref);
	return true;
}

// ---- host only: the header ----
struct Header {
	uint64_t text_at = 8, l_text = 0;   // the SAM header text
	uint64_t refs_at = 0;               // n_ref's four bytes; the reference list follows
	uint64_t end = 0;                   // the first record
	int32_t n_ref = 0;
};

// s[0 .. n): the first bytes of the inflated stream.  0: h is filled in; 1: the header is not complete in n bytes; < 0: -(offset) - 1 of
// what is no BAM header (the magic: offset 0; a negative l_text, n_ref or l_name, or an l_name of 0: that field's offset).
inline int64_t parse_header(const uint8_t *s, uint64_t n, Header &h)
{
	if (n < 4) return memcmp(s, "BAM\1", (size_t)n) ? -1 : 1;
	if (memcmp(s, "BAM\1", 4)) return -1;
	if (n < 8) return 1;
	const uint32_t l_text = load32(s, 4);
	if (l_text > 0x7fffffffu) return -4 - 1;
	h.text_at = 8; h.l_text = l_text;
	uint64_t at = 8 + (uint64_t)l_text;
	if (n < at + 4) return 1;
	const uint32_t n_ref = load32(s, at);
	if (n_ref > 0x7fffffffu) return -(int64_t)at - 1;
	h.refs_at = at; h.n_ref = (int32_t)n_ref;
	at += 4;
	for (uint32_t k = 0; k < n_ref; ++k) {
		if (n < at + 4) return 1;
		const uint32_t l_name = load32(s, at);
		if (l_name == 0 || l_name > 0x7fffffffu) return -(int64_t)at - 1;
		at += 4 + (uint64_t)l_name + 4;
		if (n < at) return 1;
	}
	h.end = at;
	return 0;
}

// The header text with SO:coordinate on its @HD line: an SO: field is replaced, an @HD line without one gets it appended, a text without
// an @HD line gets "@HD\tVN:1.6\tSO:coordinate\n" in front; every other byte stays.  (@HD counts only as the text's first line, where
// the SAM specification puts it.)
constexpr uint32_t BAM_SORT_HEADER_GROWTH = 25;   // the longest of the three: the whole line in front
inline std::string coordinate_text(const char *text, size_t len)
{
	static const char so[] = "SO:coordinate";
	const std::string t(text, len);
	if (len < 3 || memcmp(text, "@HD", 3) || (len > 3 && text[3] != '\t' && text[3] != '\n')) return std::string("@HD\tVN:1.6\t") + so + "\n" + t;
	size_t eol = t.find('\n');
	if (eol == std::string::npos) eol = len;
	for (size_t f = 3; f < eol;) {   // the fields of the line, each behind a tab at f
		size_t e = t.find('\t', f + 1);
		if (e == std::string::npos || e > eol) e = eol;
		if (e - f >= 4 && !memcmp(text + f + 1, "SO:", 3)) return t.substr(0, f + 1) + so + t.substr(e);
		f = e;
	}
	return t.substr(0, eol) + "\t" + so + t.substr(eol);
}

// the whole header (magic, l_text, text, n_ref, references) with the rewritten text; s holds the old one, h describes it
inline void coordinate_header(const uint8_t *s, const Header &h, std::vector<uint8_t> &out)
{
	const std::string text = coordinate_text((const char *)s + h.text_at, (size_t)h.l_text);
	out.resize(8 + text.size() + (size_t)(h.end - h.refs_at));
	memcpy(out.data(), "BAM\1", 4);
	const uint32_t l = (uint32_t)text.size();
	for (int k = 0; k < 4; ++k) out[4 + k] = (uint8_t)(l >> (8 * k));
	memcpy(out.data() + 8, text.data(), text.size());
	memcpy(out.data() + 8 + text.size(), s + h.refs_at, (size_t)(h.end - h.refs_at));
}

} // namespace bsort
} // namespace mbw
#endif
