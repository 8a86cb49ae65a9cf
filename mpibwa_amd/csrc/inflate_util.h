// inflate_util.h — the arithmetic of the device inflate (bgzf_inflate_kernel.hip): a complete RFC 1951 decoder that turns the deflate
// stream of one BGZF block into batches of tokens, and what a lane does with a batch and with the window.  Plain functions for host and
// device: the kernel only adds the barriers between them, so that the host can run the same source lane by lane against zlib without
// a GPU (tests/test_inflate_kernel_host.py).  DESIGN §8.3.
//
// Every loop here has a trip count that is bounded by a size known at entry (an alphabet size, 15 code lengths, IF_BATCH tokens, eight
// bytes of refill), every table index is checked or masked, and no byte of the input is read at or beyond in_len.
#ifndef MBW_INFLATE_UTIL_H
#define MBW_INFLATE_UTIL_H
#include "deflate_util.h"

namespace mbw {
namespace ifl {

constexpr uint32_t IF_WINDOW = 32768;      // the circular window: no distance exceeds it (RFC 1951 3.2.5)
constexpr uint32_t IF_WMASK = IF_WINDOW - 1;
constexpr uint32_t IF_BATCH = 64;          // tokens per batch: at most 64 * 258 = 16 512 bytes, which leaves the window's other half intact
constexpr uint32_t IF_ROW = 256;           // the window leaves for HBM in rows of 64 dwords
constexpr uint32_t IF_MAX_TEXT = 65536;    // BGZF's largest block

// the status word of a block
enum : uint32_t {
	IF_OK = 0,
	IF_E_INPUT = 1,        // the payload ran out
	IF_E_BTYPE = 2,        // block type 3
	IF_E_STORED = 3,       // LEN / NLEN mismatch
	IF_E_HEADER = 4,       // more than 286 literal/length or 30 distance codes, a repeat without a length before it or past the end, no code for 256
	IF_E_OVER = 5,         // a set of code lengths that over-subscribes
	IF_E_INCOMPLETE = 6,   // an incomplete set that zlib does not take either
	IF_E_SYMBOL = 7,       // a bit pattern that is no code, literal/length symbols 286 / 287, distance symbols 30 / 31
	IF_E_DIST = 8,         // a distance that reaches before the block's first byte
	IF_E_LONG = 9,         // more text than ISIZE
	IF_E_SHORT = 10,       // the stream ended before ISIZE
	IF_E_CRC = 11,         // the text's CRC32 is not the trailer's
	IF_E_SIZE = 12,        // ISIZE above 64 KiB (no BGZF block), found before the launch
};

// A canonical code as RFC 1951 3.2.2 defines it: count[l] codes of l bits, their symbols in symbol[] by length, then by value.
struct Huff {
	uint16_t count[16];
	uint16_t offs[16];       // huff_build's: where the symbols of a length go (kept here, not in a local array: no scratch on the device)
	uint16_t symbol[288];
};

// lens[0 .. n) -> h.  kind 0: the code-length code, 1: literal/length, 2: distance.  An over-subscribed set is refused.  An incomplete
// set is refused but for the two incompletenesses that zlib's inflate_table takes for the literal/length and distance codes: no code at
// all, and a single code of one bit (its other bit pattern is then no code: decode() refuses it when it comes).
MBW_HD uint32_t huff_build(Huff &h, const uint8_t *lens, uint32_t n, int kind)
{
	if (n > 288) return IF_E_HEADER;
	for (int l = 0; l < 16; ++l) h.count[l] = 0;
	for (uint32_t s = 0; s < n; ++s) ++h.count[lens[s] & 15u];
	int left = 1;
	for (int l = 1; l < 16; ++l) {
		left = (left << 1) - (int)h.count[l];
		if (left < 0) return IF_E_OVER;
	}
	if (left > 0) {
		const bool none = h.count[0] == n, one_bit = h.count[1] == 1 && (uint32_t)h.count[0] + 1 == n;
		if (kind == 0 || !(none || one_bit)) return IF_E_INCOMPLETE;
	}
	h.offs[0] = h.offs[1] = 0;
	for (int l = 1; l < 15; ++l) h.offs[l + 1] = (uint16_t)(h.offs[l] + h.count[l]);
	for (uint32_t s = 0; s < n; ++s) {
		const uint32_t l = lens[s] & 15u;
		if (l) { const uint32_t at = h.offs[l]++; if (at < 288) h.symbol[at] = (uint16_t)s; }
	}
	return IF_OK;
}

// lane 0's state between the batches of a block (in LDS on the device)
struct Decoder {
	const uint8_t *in;       // the deflate stream
	uint32_t in_len, next;   // its size; the next byte to enter hold
	uint64_t hold;           // bits not used yet, the next one lowest
	uint32_t nbits;
	uint32_t phase;          // 0: at a block header, 1: in a stored block, 2: in a coded block, 3: behind the last block
	uint32_t last;           // BFINAL of the block at hand
	uint32_t stored_left;
	Huff ll, d, cl;
	uint8_t lens[320];
};

MBW_HD void decoder_init(Decoder &D, const uint8_t *in, uint32_t in_len)
{
	D.in = in; D.in_len = in_len; D.next = 0; D.hold = 0; D.nbits = 0; D.phase = 0; D.last = 0; D.stored_left = 0;
}

// at least 56 bits in hold, or all that the payload still has (at most eight steps)
MBW_HD void refill(Decoder &D)
{
	for (int k = 0; k < 8 && D.nbits <= 56 && D.next < D.in_len; ++k) {
		D.hold |= (uint64_t)D.in[D.next++] << D.nbits;
		D.nbits += 8;
	}
}
// k <= 16 bits; false when the payload has run out
MBW_HD bool take(Decoder &D, uint32_t k, uint32_t &v)
{
	if (D.nbits < k) { refill(D); if (D.nbits < k) return false; }
	v = (uint32_t)D.hold & ((1u << k) - 1);
	D.hold >>= k; D.nbits -= k;
	return true;
}
// one symbol of h, a bit at a time along the canonical code (at most 15 steps).  A code that matches stands below the number of coded
// symbols (huff_build refused an over-subscribed set), so h.symbol[at] is an entry that huff_build wrote.
MBW_HD uint32_t decode(Decoder &D, const Huff &h, uint32_t &sym)
{
	if (D.nbits < 15) refill(D);
	uint32_t code = 0, first = 0, index = 0;
	for (uint32_t l = 1; l <= 15; ++l) {
		if (D.nbits < l) return IF_E_INPUT;
		code |= (uint32_t)(D.hold >> (l - 1)) & 1u;
		const uint32_t count = h.count[l];
		if (code < first + count) {
			const uint32_t at = index + (code - first);
			if (at >= 288) return IF_E_SYMBOL;
			sym = h.symbol[at];
			D.hold >>= l; D.nbits -= l;
			return IF_OK;
		}
		index += count; first = (first + count) << 1; code <<= 1;
	}
	return IF_E_SYMBOL;
}

MBW_HD uint32_t length_base(uint32_t code)   // code 257 .. 285
{
	const uint32_t c = code - 257;
	if (c < 8) return 3 + c;
	if (c == 28) return 258;
	const uint32_t nb = (c - 4) >> 2;
	return 3 + ((4 + (c & 3u)) << nb);
}
MBW_HD uint32_t dist_base(uint32_t code)   // code 0 .. 29
{
	if (code < 4) return 1 + code;
	const uint32_t nb = (code - 2) >> 1;
	return 1 + ((2 + (code & 1u)) << nb);
}

// the header of a block with dynamic codes (RFC 1951 3.2.7)
MBW_HD uint32_t read_dynamic(Decoder &D)
{
	uint32_t v;
	if (!take(D, 14, v)) return IF_E_INPUT;
	const uint32_t nlen = (v & 31u) + 257, ndist = ((v >> 5) & 31u) + 1, ncode = (v >> 10) + 4;
	if (nlen > 286 || ndist > 30) return IF_E_HEADER;
	const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
	for (uint32_t k = 0; k < 19; ++k) D.lens[k] = 0;
	for (uint32_t k = 0; k < ncode; ++k) {
		if (!take(D, 3, v)) return IF_E_INPUT;
		D.lens[order[k]] = (uint8_t)v;
	}
	uint32_t st = huff_build(D.cl, D.lens, 19, 0);
	if (st) return st;
	const uint32_t total = nlen + ndist;
	uint32_t at = 0;
	for (uint32_t step = 0; step < 320 && at < total; ++step) {   // (every step adds at least one length)
		uint32_t sym;
		st = decode(D, D.cl, sym);
		if (st) return st;
		if (sym < 16) { D.lens[at++] = (uint8_t)sym; continue; }
		uint32_t prev = 0, rep;
		if (sym == 16) {
			if (!at) return IF_E_HEADER;
			prev = D.lens[at - 1];
			if (!take(D, 2, v)) return IF_E_INPUT;
			rep = 3 + v;
		} else if (sym == 17) {
			if (!take(D, 3, v)) return IF_E_INPUT;
			rep = 3 + v;
		} else {
			if (!take(D, 7, v)) return IF_E_INPUT;
			rep = 11 + v;
		}
		if (at + rep > total) return IF_E_HEADER;   // (a run may cross from the literal/length lengths into the distance lengths, not past them)
		for (uint32_t k = 0; k < rep; ++k) D.lens[at++] = (uint8_t)prev;
	}
	if (D.lens[256] == 0) return IF_E_HEADER;
	st = huff_build(D.ll, D.lens, nlen, 1);
	if (st) return st;
	return huff_build(D.d, D.lens + nlen, ndist, 2);
}

MBW_HD uint32_t read_fixed(Decoder &D)
{
	for (uint32_t s = 0; s < 288; ++s) D.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
	for (uint32_t s = 0; s < 32; ++s) D.lens[288 + s] = 5;
	uint32_t st = huff_build(D.ll, D.lens, 288, 1);
	if (st) return st;
	return huff_build(D.d, D.lens + 288, 32, 2);   // (all 32 five-bit codes, as RFC 1951 3.2.6 has them: decode_batch refuses symbols 30 and 31)
}

// Lane 0: the next tokens of the block, at most IF_BATCH.  A token is a literal (its byte, bits 16.. zero) or a match (length << 16 |
// distance, distance 1 .. 32 768).  pos: bytes of text before this batch; isize: the text's size by the trailer.  n_tok and n_bytes
// describe the batch; *done is set behind the last block.  A call consumes at least one bit of the payload, returns an error or sets
// *done, so a block takes at most 8 * in_len + 1 calls.
MBW_HD uint32_t decode_batch(Decoder &D, uint32_t pos, uint32_t isize, uint32_t *tok, uint32_t &n_tok, uint32_t &n_bytes, uint32_t &done)
{
	n_tok = 0; n_bytes = 0; done = 0;
	for (uint32_t step = 0; step < 4 * IF_BATCH && n_tok < IF_BATCH; ++step) {   // (steps without a token: block headers and ends; the batch closes early after 4 * IF_BATCH steps)
		uint32_t v;
		if (D.phase == 3) { done = 1; return IF_OK; }
		if (D.phase == 0) {
			if (!take(D, 3, v)) return IF_E_INPUT;
			D.last = v & 1u;
			const uint32_t type = v >> 1;
			if (type == 3) return IF_E_BTYPE;
			if (type == 0) {
				const uint32_t drop = D.nbits & 7u;   // to the byte boundary (hold's bits end at one)
				D.hold >>= drop; D.nbits -= drop;
				uint32_t a, b;
				if (!take(D, 16, a) || !take(D, 16, b)) return IF_E_INPUT;
				if ((a ^ b) != 0xffffu) return IF_E_STORED;
				D.stored_left = a;
				D.phase = 1;
			} else {
				const uint32_t st = type == 1 ? read_fixed(D) : read_dynamic(D);
				if (st) return st;
				D.phase = 2;
			}
			continue;
		}
		if (D.phase == 1) {
			if (!D.stored_left) { D.phase = D.last ? 3 : 0; continue; }
			if (!take(D, 8, v)) return IF_E_INPUT;
			if (pos + n_bytes + 1 > isize) return IF_E_LONG;
			tok[n_tok++] = v; ++n_bytes; --D.stored_left;
			continue;
		}
		uint32_t sym;
		uint32_t st = decode(D, D.ll, sym);
		if (st) return st;
		if (sym < 256) {
			if (pos + n_bytes + 1 > isize) return IF_E_LONG;
			tok[n_tok++] = sym; ++n_bytes;
			continue;
		}
		if (sym == 256) { D.phase = D.last ? 3 : 0; continue; }
		if (sym > 285) return IF_E_SYMBOL;
		uint32_t len = length_base(sym);
		const uint32_t lnb = dfl::len_extra_bits(sym);
		if (lnb) { if (!take(D, lnb, v)) return IF_E_INPUT; len += v; }
		st = decode(D, D.d, sym);
		if (st) return st;
		if (sym > 29) return IF_E_SYMBOL;
		uint32_t dist = dist_base(sym);
		const uint32_t dnb = dfl::dist_extra_bits(sym);
		if (dnb) { if (!take(D, dnb, v)) return IF_E_INPUT; dist += v; }
		if (dist > pos + n_bytes) return IF_E_DIST;
		if (pos + n_bytes + len > isize) return IF_E_LONG;
		tok[n_tok++] = len << 16 | dist; n_bytes += len;
	}
	if (D.phase == 3) done = 1;
	return IF_OK;
}

// ---- what every lane does ----
MBW_HD uint32_t tok_len(uint32_t t) { return t >> 16 ? t >> 16 : 1u; }

// A lane's bytes of the match token t whose first byte stands at text position `at`: bytes lane, lane + 64, ... of the match.  The
// source is the `dist` bytes before `at`, taken round and round (k mod dist), so that a match that overlaps its own output comes out
// right whatever the order of the lanes: nothing that this token writes is read for it.
MBW_HD void place_match(uint8_t *win, uint32_t at, uint32_t t, uint32_t lane)
{
	const uint32_t len = t >> 16, dist = t & 0xffffu;   // (decode_batch: 3 <= len <= 258, 1 <= dist <= 32 768)
	for (uint32_t k = lane; k < len && k < 258; k += 64) win[(at + k) & IF_WMASK] = win[(at - dist + k % dist) & IF_WMASK];
}

// A lane's share of the row of IF_ROW bytes at text position `row` (a multiple of IF_ROW): bytes lane, lane + 64, ... go to out (the
// block's text, out[row + j] with row + j < isize by the caller's bound), dword `lane` enters the lane's CRC register by a Horner step.
MBW_HD void flush_row(const uint8_t *win, uint32_t row, uint8_t *out, uint32_t lane, uint32_t x2048, uint32_t &acc)
{
	const uint32_t w = (row & IF_WMASK) + 4 * lane;
	for (uint32_t k = 0; k < 4; ++k) out[row + 64 * k + lane] = win[(row + 64 * k + lane) & IF_WMASK];
	const uint32_t d = (uint32_t)win[w] | (uint32_t)win[w + 1] << 8 | (uint32_t)win[w + 2] << 16 | (uint32_t)win[w + 3] << 24;
	acc = dfl::gf_mul(acc, x2048) ^ d;
}

// The lane's part of the raw CRC of the n bytes of text, after all whole rows went through flush_row and with the last n mod IF_ROW
// bytes still in the window; it also writes those bytes to out.  The parts of the 64 lanes xor-ed together are the raw CRC.
MBW_HD uint32_t flush_tail(const uint8_t *win, uint32_t n, uint8_t *out, uint32_t lane, const uint32_t x2n[32], uint32_t acc)
{
	const uint32_t rows = n / IF_ROW, tail = n % IF_ROW, base = rows * IF_ROW;
	uint32_t part = 0;
	// the lane's dwords of the rows: the last one has 252 - 4 * lane bytes of its row and the tail behind it
	if (rows) part = dfl::gf_mul(acc, dfl::gf_xpow(x2n, 32u + 8u * (IF_ROW - 4 - 4 * lane + tail)));
	for (uint32_t j = lane; j < tail; j += 64) out[base + j] = win[(base + j) & IF_WMASK];
	const uint32_t nd = tail >> 2, tb = tail & 3u;
	if (lane < nd) {
		const uint32_t w = (base & IF_WMASK) + 4 * lane;
		const uint32_t d = (uint32_t)win[w] | (uint32_t)win[w + 1] << 8 | (uint32_t)win[w + 2] << 16 | (uint32_t)win[w + 3] << 24;
		part ^= dfl::gf_mul(d, dfl::gf_xpow(x2n, 32u + 8u * (tail - 4 - 4 * lane)));
	}
	if (lane == 0 && tb) {
		uint32_t t = 0;
		for (uint32_t k = 0; k < tb; ++k) t |= (uint32_t)win[(base + 4 * nd + k) & IF_WMASK] << (8 * k);
		part ^= dfl::gf_mul(t, dfl::gf_xpow(x2n, 8u * tb));
	}
	return part;
}

} // namespace ifl
} // namespace mbw
#endif
