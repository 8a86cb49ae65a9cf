// bam_util.h — one SAM line to one BAM record, the arithmetic that does not need a wavefront: where the fields stand, the numbers, the
// contig lookup, reg2bin, the CIGAR words, the SEQ nibbles, the tags and the record's size.  Plain functions for host and device, so
// that sampost.cpp (mi355x_sam_to_bam) and bam_kernel.hip (mi355x_sam_to_bam_dev) state the layout once and the CPU suite checks it
// without a GPU.  DESIGN §8.4.
//
// A record (little-endian): int32 block_size | int32 refID | int32 pos | uint8 l_read_name | uint8 mapq | uint16 bin | uint16 n_cigar_op |
// uint16 flag | int32 l_seq | int32 next_refID | int32 next_pos | int32 tlen | QNAME NUL | n_cigar_op x uint32 (len << 4 | op) |
// (l_seq + 1) / 2 bytes of SEQ nibbles | l_seq bytes of QUAL - 33 (0xff: QUAL '*') | tags.
//
// Every line gets one of three verdicts: BAM_OK, BAM_DECLINE (well-formed, but only the host build of this header encodes it: a 'B' tag,
// a float that is not digits '.' 1-6 digits, a record above 0xff00 bytes) or BAM_ERROR (malformed text, or text that no BAM record holds:
// a QNAME above 254 bytes, more than 65 535 CIGAR operations, an integer tag outside -2^31 .. 2^32 - 1).
#ifndef MBW_BAM_UTIL_H
#define MBW_BAM_UTIL_H
#include <stdint.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <stdlib.h>
#include <string.h>
#endif

#if defined(__HIPCC__)
#define MBW_BAM_HD __host__ __device__ inline
#else
#define MBW_BAM_HD inline
#endif

namespace mbw {
namespace bam {

enum : int { BAM_OK = 0, BAM_DECLINE = 1, BAM_ERROR = 2 };
constexpr uint32_t BAM_BLOCK_INPUT = 0xff00;   // BAM bytes per BGZF block (sampost.cpp: BGZF_INPUT)
constexpr uint32_t BAM_MIN_LINE = 22;          // eleven fields of one byte, ten tabs, the newline

// The contig table both sides look RNAME / RNEXT up in: the names sorted bytewise (equal names by index, so that the first of them is
// found, as ContigIndex of sampost.cpp finds it), in one blob that travels to the device as it is:
//   int32 n | int32 id[n] | uint32 off[n + 1] | the names back to back (sorted order, no NUL)
struct ContigTable {
	const int32_t *id = nullptr;
	const uint32_t *off = nullptr;
	const uint8_t *names = nullptr;
	int n = 0;
};
MBW_BAM_HD ContigTable contig_table_at(const void *blob)
{
	ContigTable t;
	const int32_t *w = (const int32_t *)blob;
	t.n = w[0];
	t.id = w + 1;
	t.off = (const uint32_t *)(w + 1 + t.n);
	t.names = (const uint8_t *)(t.off + t.n + 1);
	return t;
}
// < 0, 0, > 0 as memcmp on the common length, then the shorter first
MBW_BAM_HD int name_cmp(const uint8_t *a, uint32_t na, const uint8_t *b, uint32_t nb)
{
	const uint32_t n = na < nb ? na : nb;
	for (uint32_t k = 0; k < n; ++k)
		if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
	return na < nb ? -1 : na > nb ? 1 : 0;
}
// index of the first contig of that name, -1: none
MBW_BAM_HD int contig_find(const ContigTable &t, const uint8_t *s, uint32_t n)
{
	int lo = 0, hi = t.n;   // the first entry that is not below s
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (name_cmp(t.names + t.off[mid], t.off[mid + 1] - t.off[mid], s, n) < 0) lo = mid + 1; else hi = mid;
	}
	if (lo < t.n && name_cmp(t.names + t.off[lo], t.off[lo + 1] - t.off[lo], s, n) == 0) return t.id[lo];
	return -1;
}

// what the size pass knows about a line and the write pass needs: offsets are from the line's first byte
struct LinePlan {
	uint32_t size;        // the whole record, block_size's four bytes included; 0 unless the verdict is BAM_OK
	int32_t refid, pos, next_refid, next_pos, tlen, l_seq;
	uint32_t o_cigar, n_cigar_text, o_seq, o_qual, o_tags, n_line;   // CIGAR field and its length; SEQ; QUAL; first tag (n_line: none); line length without '\n'
	uint16_t flag, n_cigar, bin;
	uint8_t mapq, l_qname, qual_star;
};

// digits only, at least one, value <= max
MBW_BAM_HD bool parse_uint(const uint8_t *s, uint32_t a, uint32_t b, uint64_t max, uint64_t &v)
{
	if (a >= b || b - a > 19) return false;
	v = 0;
	for (uint32_t k = a; k < b; ++k) {
		if (s[k] < '0' || s[k] > '9') return false;
		v = v * 10 + (uint64_t)(s[k] - '0');
	}
	return v <= max;
}
// an optional '-' or '+', then digits: lo <= value <= hi (|lo|, hi < 2^63)
MBW_BAM_HD bool parse_int(const uint8_t *s, uint32_t a, uint32_t b, int64_t lo, int64_t hi, int64_t &v)
{
	bool neg = false;
	if (a < b && (s[a] == '-' || s[a] == '+')) neg = s[a++] == '-';
	uint64_t u;
	if (!parse_uint(s, a, b, neg ? (uint64_t)(-(lo + 1)) + 1 : (uint64_t)hi, u)) return false;
	v = neg ? -(int64_t)u : (int64_t)u;
	return lo <= 0 || v >= lo;
}

// reg2bin on [beg, end): the first level at which both ends fall into one bin; the shifts are arithmetic (POS 0: beg = -1 gives 4680)
MBW_BAM_HD uint16_t reg2bin(int64_t beg, int64_t end)
{
	--end;
	for (int k = 14; k <= 26; k += 3)
		if ((beg >> k) == (end >> k)) return (uint16_t)((((1 << (29 - k)) - 1) / 7) + (beg >> k));
	return 0;
}

MBW_BAM_HD int cigar_op(uint8_t c)
{
	switch (c) {
	case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
	case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
	}
	return -1;
}
// the CIGAR field s[a .. b) ('*': no operations): its words to out (or nowhere), the operations and the reference bases they cover
MBW_BAM_HD bool cigar_walk(const uint8_t *s, uint32_t a, uint32_t b, uint8_t *out, uint32_t &n_ops, int64_t &ref_len)
{
	n_ops = 0; ref_len = 0;
	if (b - a == 1 && s[a] == '*') return true;
	while (a < b) {
		uint64_t len = 0;
		uint32_t d = 0;
		for (; a < b && s[a] >= '0' && s[a] <= '9'; ++a, ++d) {
			len = len * 10 + (uint64_t)(s[a] - '0');
			if (len > 0x0fffffffu) return false;
		}
		if (!d || a >= b) return false;
		const int op = cigar_op(s[a++]);
		if (op < 0) return false;
		if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += (int64_t)len;
		if (out) {
			const uint32_t w = (uint32_t)len << 4 | (uint32_t)op;
			for (int k = 0; k < 4; ++k) out[4 * n_ops + k] = (uint8_t)(w >> (8 * k));
		}
		++n_ops;
	}
	return true;
}

// "=ACMGRSVTWYHKDBN" -> 0 .. 15, lower case as upper case, anything else 15
MBW_BAM_HD uint32_t seq_nibble(uint8_t c)
{
	switch (c & 0xdf) {   // (letters: upper case; '=' (0x3d) is handled first)
	case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
	case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
	}
	return 15;
}
MBW_BAM_HD uint32_t seq_code(uint8_t c) { return c == '=' ? 0u : ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) ? seq_nibble(c) : 15u; }
// byte k of the packed SEQ: bases 2k (high nibble) and 2k + 1 (0 behind an odd end)
MBW_BAM_HD uint8_t seq_byte(const uint8_t *seq, uint32_t l_seq, uint32_t k)
{
	const uint32_t hi = seq_code(seq[2 * k]), lo = 2 * k + 1 < l_seq ? seq_code(seq[2 * k + 1]) : 0u;
	return (uint8_t)(hi << 4 | lo);
}

// The float32 nearest to sign digits '.' 1-6 digits (ties to even), by integer long division: the value is N / 10^k with N < 10^15, so
// every intermediate fits 64 bits and no double stands on the way.  false: the text has another form (the host then asks strtof).
MBW_BAM_HD bool plain_float_bits(const uint8_t *s, uint32_t a, uint32_t b, uint32_t &bits)
{
	uint32_t sign = 0;
	if (a < b && (s[a] == '-' || s[a] == '+')) sign = s[a++] == '-' ? 0x80000000u : 0u;
	uint64_t N = 0, D = 1;
	uint32_t nd = 0, nf = 0;
	bool point = false;
	for (; a < b; ++a) {
		if (s[a] == '.') { if (point || !nd) return false; point = true; continue; }
		if (s[a] < '0' || s[a] > '9') return false;
		N = N * 10 + (uint64_t)(s[a] - '0');
		if (point) { ++nf; D *= 10; } else ++nd;
		if (nd + nf > 15 || nf > 6) return false;
	}
	if (!point || !nf) return false;
	if (!N) { bits = sign; return true; }
	// q = floor(N * 2^sh / D) with 2^24 <= q < 2^25: 24 bits of the result and a guard bit; the remainder is the sticky bit
	int sh = 0;
	uint64_t num = N, den = D;
	while (num / den >= (1ull << 25)) { den <<= 1; --sh; }     // (den < 2^20 * 2^26)
	while (num / den < (1ull << 24)) { num <<= 1; ++sh; }      // (num < 2^25 * den <= 2^45 * 2^0 .. : below 2^64)
	const uint64_t q = num / den, rem = num % den;
	uint64_t m = q >> 1;
	if ((q & 1) && (rem || (m & 1))) ++m;
	int e = 1 - sh + 23;   // value = q * 2^-sh = (q / 2) * 2^(1 - sh); m in [2^23, 2^24] carries the exponent 23
	if (m == (1ull << 24)) { m >>= 1; ++e; }
	bits = sign | (uint32_t)(e + 127) << 23 | ((uint32_t)m & 0x7fffffu);
	return true;
}

MBW_BAM_HD void put16(uint8_t *o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); }
MBW_BAM_HD void put32(uint8_t *o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24); }

// an integer value in the smallest type that holds it, unsigned when it is not negative: the type letter and the bytes behind it
MBW_BAM_HD uint32_t put_int_tag(int64_t v, uint8_t *out)
{
	uint8_t t;
	uint32_t n;
	if (v >= 0) { if (v <= 255) { t = 'C'; n = 1; } else if (v <= 65535) { t = 'S'; n = 2; } else { t = 'I'; n = 4; } }
	else { if (v >= -128) { t = 'c'; n = 1; } else if (v >= -32768) { t = 's'; n = 2; } else { t = 'i'; n = 4; } }
	if (out) {
		out[0] = t;
		for (uint32_t k = 0; k < n; ++k) out[1 + k] = (uint8_t)((uint64_t)v >> (8 * k));
	}
	return 1 + n;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// host only: any float strtof takes whole
inline bool any_float_bits(const uint8_t *s, uint32_t a, uint32_t b, uint32_t &bits)
{
	if (a >= b || b - a > 63) return false;
	char buf[64];
	memcpy(buf, s + a, b - a);
	buf[b - a] = 0;
	if (buf[0] == ' ' || buf[0] == '\t') return false;
	char *end = nullptr;
	const float f = strtof(buf, &end);
	if (end != buf + (b - a)) return false;
	memcpy(&bits, &f, 4);
	return true;
}
// host only: the value of a 'B' tag, s[a .. b) = subtype [',' element]*; returns its bytes (subtype, count, elements) or 0: malformed
inline uint32_t put_array_tag(const uint8_t *s, uint32_t a, uint32_t b, uint8_t *out)
{
	if (a >= b) return 0;
	const uint8_t sub = s[a++];
	uint32_t width;
	int64_t lo = 0, hi = 0;
	switch (sub) {
	case 'c': width = 1; lo = -128; hi = 127; break;
	case 'C': width = 1; hi = 255; break;
	case 's': width = 2; lo = -32768; hi = 32767; break;
	case 'S': width = 2; hi = 65535; break;
	case 'i': width = 4; lo = -2147483648ll; hi = 2147483647ll; break;
	case 'I': width = 4; hi = 4294967295ll; break;
	case 'f': width = 4; break;
	default: return 0;
	}
	uint32_t count = 0, w = 5;
	while (a < b) {
		if (s[a++] != ',') return 0;
		uint32_t e = a;
		while (e < b && s[e] != ',') ++e;
		uint32_t bits;
		if (sub == 'f') {
			if (!plain_float_bits(s, a, e, bits) && !any_float_bits(s, a, e, bits)) return 0;
		} else {
			int64_t v;
			if (!parse_int(s, a, e, lo, hi, v)) return 0;
			bits = (uint32_t)v;
		}
		if (out)
			for (uint32_t k = 0; k < width; ++k) out[w + k] = (uint8_t)(bits >> (8 * k));
		w += width; ++count; a = e;
	}
	if (out) { out[0] = sub; put32(out + 1, count); }
	return w;
}
#endif

// The tags s[a .. n) (tab-separated NN:T:value) to out, or nowhere when out is null; returns their bytes and the verdict.
MBW_BAM_HD uint32_t tags_walk(const uint8_t *s, uint32_t a, uint32_t n, uint8_t *out, int &verdict)
{
	uint32_t w = 0;
	verdict = BAM_OK;
	while (a < n) {
		uint32_t e = a;
		while (e < n && s[e] != '\t') ++e;
		if (e - a < 5 || s[a + 2] != ':' || s[a + 4] != ':') { verdict = BAM_ERROR; return 0; }
		const uint8_t type = s[a + 3];
		const uint32_t v0 = a + 5;
		uint8_t *o = out ? out + w : nullptr;
		if (o) { o[0] = s[a]; o[1] = s[a + 1]; }
		w += 2;
		if (o) o += 2;
		if (type == 'A') {
			if (e - v0 != 1) { verdict = BAM_ERROR; return 0; }
			if (o) { o[0] = 'A'; o[1] = s[v0]; }
			w += 2;
		} else if (type == 'i') {
			int64_t v;
			if (!parse_int(s, v0, e, -2147483648ll, 4294967295ll, v)) { verdict = BAM_ERROR; return 0; }
			w += put_int_tag(v, o);
		} else if (type == 'Z' || type == 'H') {
			if (o) {
				o[0] = type;
				for (uint32_t k = v0; k < e; ++k) o[1 + k - v0] = s[k];
				o[1 + e - v0] = 0;
			}
			w += 2 + (e - v0);
		} else if (type == 'f') {
			uint32_t bits;
			if (!plain_float_bits(s, v0, e, bits)) {
#if defined(__HIP_DEVICE_COMPILE__)
				verdict = BAM_DECLINE; return 0;
#else
				if (!any_float_bits(s, v0, e, bits)) { verdict = BAM_ERROR; return 0; }
#endif
			}
			if (o) { o[0] = 'f'; put32(o + 1, bits); }
			w += 5;
		} else if (type == 'B') {
#if defined(__HIP_DEVICE_COMPILE__)
			verdict = BAM_DECLINE; return 0;
#else
			const uint32_t k = put_array_tag(s, v0, e, o ? o + 1 : nullptr);
			if (!k) { verdict = BAM_ERROR; return 0; }
			if (o) o[0] = 'B';
			w += 1 + k;
#endif
		} else { verdict = BAM_ERROR; return 0; }
		a = e + 1;
		if (e < n && a == n) { verdict = BAM_ERROR; return 0; }   // a tab at the line's end
	}
	return w;
}

// The size pass of one line s[0 .. n) (without its '\n').  P.size is 0 unless the verdict is BAM_OK.
MBW_BAM_HD int plan_line(const uint8_t *s, uint32_t n, const ContigTable &tab, LinePlan &P)
{
	P.size = 0; P.n_line = n;
	uint32_t f0[11], f1[11];
	uint32_t at = 0;
	for (int f = 0; f < 11; ++f) {
		if (at > n) return BAM_ERROR;      // fewer than 11 fields
		uint32_t e = at;
		while (e < n && s[e] != '\t') ++e;
		if (e == at) return BAM_ERROR;     // an empty field
		f0[f] = at; f1[f] = e;
		at = e + 1;
	}
	if (at == n) return BAM_ERROR;         // a tab behind QUAL and nothing after it
	P.o_tags = at < n ? at : n;
	if (f1[0] - f0[0] > 254) return BAM_ERROR;
	P.l_qname = (uint8_t)(f1[0] - f0[0] + 1);
	uint64_t u;
	int64_t v;
	if (!parse_uint(s, f0[1], f1[1], 65535, u)) return BAM_ERROR;
	P.flag = (uint16_t)u;
	if (f1[2] - f0[2] == 1 && s[f0[2]] == '*') P.refid = -1;
	else if ((P.refid = contig_find(tab, s + f0[2], f1[2] - f0[2])) < 0) return BAM_ERROR;
	if (!parse_uint(s, f0[3], f1[3], 2147483647u, u)) return BAM_ERROR;
	P.pos = (int32_t)u - 1;
	if (!parse_uint(s, f0[4], f1[4], 255, u)) return BAM_ERROR;
	P.mapq = (uint8_t)u;
	uint32_t n_ops;
	int64_t ref_len;
	if (!cigar_walk(s, f0[5], f1[5], nullptr, n_ops, ref_len) || n_ops > 65535) return BAM_ERROR;
	P.o_cigar = f0[5]; P.n_cigar_text = f1[5] - f0[5]; P.n_cigar = (uint16_t)n_ops;
	if (f1[6] - f0[6] == 1 && s[f0[6]] == '=') P.next_refid = P.refid;
	else if (f1[6] - f0[6] == 1 && s[f0[6]] == '*') P.next_refid = -1;
	else if ((P.next_refid = contig_find(tab, s + f0[6], f1[6] - f0[6])) < 0) return BAM_ERROR;
	if (!parse_uint(s, f0[7], f1[7], 2147483647u, u)) return BAM_ERROR;
	P.next_pos = (int32_t)u - 1;
	if (!parse_int(s, f0[8], f1[8], -2147483648ll, 2147483647ll, v)) return BAM_ERROR;
	P.tlen = (int32_t)v;
	P.o_seq = f0[9]; P.o_qual = f0[10];
	P.l_seq = (f1[9] - f0[9] == 1 && s[f0[9]] == '*') ? 0 : (int32_t)(f1[9] - f0[9]);
	P.qual_star = f1[10] - f0[10] == 1 && s[f0[10]] == '*';
	if (!P.qual_star && (int32_t)(f1[10] - f0[10]) != P.l_seq) return BAM_ERROR;
	P.bin = reg2bin((int64_t)P.pos, (int64_t)P.pos + (ref_len ? ref_len : 1));
	int verdict;
	const uint32_t n_tags = tags_walk(s, P.o_tags, n, nullptr, verdict);
	if (verdict != BAM_OK) return verdict;
	const uint64_t size = 36ull + P.l_qname + 4ull * P.n_cigar + ((uint64_t)P.l_seq + 1) / 2 + (uint64_t)P.l_seq + n_tags;
#if defined(__HIP_DEVICE_COMPILE__)
	if (size > BAM_BLOCK_INPUT) return BAM_DECLINE;
#else
	if (size > 0x7fffffffull) return BAM_ERROR;
#endif
	P.size = (uint32_t)size;
	return BAM_OK;
}

// where the parts of the record stand behind its first byte
MBW_BAM_HD uint32_t rec_cigar_at(const LinePlan &P) { return 36u + P.l_qname; }
MBW_BAM_HD uint32_t rec_seq_at(const LinePlan &P) { return rec_cigar_at(P) + 4u * P.n_cigar; }
MBW_BAM_HD uint32_t rec_qual_at(const LinePlan &P) { return rec_seq_at(P) + ((uint32_t)P.l_seq + 1) / 2; }
MBW_BAM_HD uint32_t rec_tags_at(const LinePlan &P) { return rec_qual_at(P) + (uint32_t)P.l_seq; }

// everything of the record but SEQ and QUAL (the device shares those two among the lanes of a wavefront)
MBW_BAM_HD void write_frame(const uint8_t *s, const LinePlan &P, uint8_t *out)
{
	put32(out, P.size - 4);
	put32(out + 4, (uint32_t)P.refid);
	put32(out + 8, (uint32_t)P.pos);
	out[12] = P.l_qname; out[13] = P.mapq;
	put16(out + 14, P.bin); put16(out + 16, P.n_cigar); put16(out + 18, P.flag);
	put32(out + 20, (uint32_t)P.l_seq);
	put32(out + 24, (uint32_t)P.next_refid);
	put32(out + 28, (uint32_t)P.next_pos);
	put32(out + 32, (uint32_t)P.tlen);
	for (uint32_t k = 0; k + 1 < P.l_qname; ++k) out[36 + k] = s[k];
	out[36 + P.l_qname - 1] = 0;
	uint32_t n_ops;
	int64_t ref_len;
	cigar_walk(s, P.o_cigar, P.o_cigar + P.n_cigar_text, out + rec_cigar_at(P), n_ops, ref_len);
	int verdict;
	tags_walk(s, P.o_tags, P.n_line, out + rec_tags_at(P), verdict);
}
MBW_BAM_HD uint8_t qual_byte(const uint8_t *s, const LinePlan &P, uint32_t k) { return P.qual_star ? (uint8_t)0xff : (uint8_t)(s[P.o_qual + k] - 33); }
// the whole record, one thread
MBW_BAM_HD void write_record(const uint8_t *s, const LinePlan &P, uint8_t *out)
{
	write_frame(s, P, out);
	uint8_t *q = out + rec_seq_at(P);
	for (uint32_t k = 0; k < ((uint32_t)P.l_seq + 1) / 2; ++k) q[k] = seq_byte(s + P.o_seq, (uint32_t)P.l_seq, k);
	q = out + rec_qual_at(P);
	for (uint32_t k = 0; k < (uint32_t)P.l_seq; ++k) q[k] = qual_byte(s, P, k);
}

// The cut rule of both BAM paths, bgzf_cuts' rule on record ends: off[0 .. n] are the records' starts and the stream's end; a block that
// starts at record i ends before the last record j > i with off[j] - off[i] <= BAM_BLOCK_INPUT.  Returns that j, or i when record i alone
// is larger than a block (the host then cuts it into blocks of BAM_BLOCK_INPUT bytes; the device has declined it).
template <class T> MBW_BAM_HD uint32_t last_fit(const T *off, uint32_t n, uint32_t i)
{
	const T limit = off[i] + BAM_BLOCK_INPUT;
	uint32_t lo = i, hi = n;   // off[lo] <= limit always
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1) >> 1;
		if (off[mid] <= limit) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// Room for the records of sam_len bytes of SAM text.  Field by field, every separator counted with the field in front of it:
//   QNAME            n + 1 text bytes -> n + 1 (the NUL)
//   FLAG RNAME POS MAPQ RNEXT PNEXT TLEN   at least 14 text bytes -> the 36 fixed bytes (block_size and the core): 8 more than twice the text
//   CIGAR            "*\t" -> 0; an operation of two text bytes ("1M") -> 4: twice the text
//   SEQ, QUAL        n + 1 and n + 1 -> (n + 1) / 2 and n; with QUAL '*': n + 3 text bytes -> (n + 1) / 2 + n <= 1.5 n + 0.5
//   tags             A: 7 -> 4; i: at least 7 -> at most 8 ("\tXX:i:-99999" is 12 -> 7); f: at least 7 -> 7; Z, H: 6 + n -> 4 + n;
//                    B: "\tXX:B:c" 7 -> 8, an element of two text bytes (",1") -> at most 4: twice the text
// so a line of L bytes gives at most 2 L + 8 bytes, and there are at most sam_len / 22 lines.
MBW_BAM_HD uint64_t records_bound(uint64_t sam_len) { return 2 * sam_len + 8 * (sam_len / BAM_MIN_LINE + 1); }

} // namespace bam
} // namespace mbw
#endif
