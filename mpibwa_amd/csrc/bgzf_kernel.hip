// bgzf_kernel.hip — BGZF blocks made on the device: a raw-deflate encoder (LZ77 matches, dynamic Huffman codes, stored fallback) that
// turns one block of SAM text into one complete BGZF block (the layout of bgzf_block() in sampost.cpp: 18-byte gzip header with the
// 'BC' field, deflate stream, CRC32, ISIZE), and the kernel that closes the 64-KiB slots up.  DESIGN §8.2.
//
// A workgroup is ONE wavefront and takes one block at a time.  Nothing here depends on what else runs on the chip: every LDS word that
// several lanes write is written with a commutative atomic (max for the hash table, add for the histograms, or for the bit stream, xor
// for the CRC), so the same text gives the same bytes on every call.  Cross-lane operations (ballot, shuffle, readfirstlane) stand in
// wave-uniform code only.
//
//   1. CRC32: lane i takes the dwords i, i + 64, ... of the block (coalesced), a Horner step in GF(2)[x] / p per dword, the lanes'
//      registers are moved to their places with x^(8 * bytes behind) and xor-ed together (deflate_util.h).
//   2. Matching, 64 positions per step: every lane hashes the 4 bytes at its position and looks up the candidate that EARLIER steps
//      left in the table, then puts its own position in with atomicMax (the largest position wins whatever the order).  A candidate
//      more than 32 768 bytes back is refused, the others are compared byte for byte (up to 258, never past the block's end).  The
//      tokens of the step are chosen greedily over the window by a scalar walk along the ballot of the lanes that have a match; a
//      match may run into the next windows (carry).  Tokens go to a global scratch of 16-bit words — a literal is one word, a match
//      two (length, distance) — and into the histograms.
//   3. Code lengths for the literal/length (286), distance (30) and code-length (19) alphabets: rank sort by all lanes, then
//      huff_lengths() on lane 0 (at most 15 / 15 / 7 bits), canonical codes by all lanes.
//   4. Coded size against stored size; the stream: header, the 316 code lengths (no run-length symbols), then one token word per
//      lane and step: bit positions by a prefix sum over the lanes, the words or-ed into an LDS window, whole dwords flushed to the slot.
#include "hip_util.h"
#include "device.h"
#include "deflate_util.h"

namespace mbw {
namespace {

constexpr int BZ_HASH_BITS = 13;
constexpr int BZ_HASH_SIZE = 1 << BZ_HASH_BITS;
constexpr uint32_t BZ_MIN_MATCH = 4, BZ_MAX_MATCH = 258, BZ_MAX_DIST = 32768;
constexpr int BZ_NLL = 286, BZ_ND = 30, BZ_NCL = 19;
constexpr uint32_t BZ_SLOT = 0x10000, BZ_HEAD = 18, BZ_TAIL = 8;

struct BzShared {
	uint32_t table[BZ_HASH_SIZE];        // position + 1 of the last occurrence of a hash, 0 = none
	uint32_t freq_ll[288], freq_d[32], freq_cl[32];
	uint32_t code_ll[288], code_d[32], code_cl[32];   // bit-reversed code | length << 16
	uint8_t len_ll[288], len_d[32], len_cl[32];
	uint32_t sorted[288], work[288], num[36];
	uint32_t stage[64];                  // the bit stream's window: whole dwords leave it for the slot
	uint32_t wlen[64];                   // match length per position of the window
	uint32_t x2n[32];                    // x^(2^k) mod the CRC polynomial
	uint32_t n_used, bits, crc;
};

// the four bytes at byte address a, from two aligned dwords (the text's buffer has slack behind its end)
__device__ inline uint32_t ld32(const uint8_t *a)
{
	const uintptr_t u = (uintptr_t)a;
	const uint32_t *w = (const uint32_t *)(u & ~(uintptr_t)3);
	const uint64_t v = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
	return (uint32_t)(v >> (8u * (uint32_t)(u & 3)));
}
__device__ inline uint64_t lowmask(uint32_t k) { return k >= 64 ? ~0ull : (1ull << k) - 1; }

// inclusive prefix sum over the wavefront; uniform code only
__device__ inline uint32_t wave_scan(uint32_t x, int lane)
{
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = (uint32_t)__shfl_up((int)x, d, 64);
		x += t & (0u - (uint32_t)(lane >= d));
	}
	return x;
}

// The wave appends nb bits (<= 32, may be 0) of val per lane, in lane order, to the stream that stands at bit *pos of the slot.
// Uniform code only.  The window S.stage[] starts at dword *pos / 32 and holds that dword's bits so far.
__device__ inline void emit(BzShared &S, uint32_t *slot32, uint32_t &pos, uint32_t val, uint32_t nb, int lane)
{
	const uint32_t incl = wave_scan(nb, lane);
	const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
	const uint32_t w0 = pos >> 5, at = pos + incl - nb;
	if (nb) {
		const uint64_t v = (uint64_t)val << (at & 31u);
		atomicOr(&S.stage[(at >> 5) - w0], (uint32_t)v);
		if ((uint32_t)(v >> 32)) atomicOr(&S.stage[(at >> 5) - w0 + 1], (uint32_t)(v >> 32));
	}
	__syncthreads();
	pos += total;
	const uint32_t done = (pos >> 5) - w0;   // whole dwords (< 64: a step appends at most 64 * 28 bits)
	const uint32_t mine = S.stage[lane], part = S.stage[done];
	if ((uint32_t)lane < done) slot32[w0 + lane] = mine;
	__syncthreads();
	S.stage[lane] = lane == 0 ? part : 0u;
	__syncthreads();
}

// used symbols of freq[0 .. n) sorted into S.sorted (frequency << 9 | symbol, ascending), at least two of them (an alphabet with fewer
// gets symbols of frequency 1, as zlib does: every decoder takes a complete code); then their lengths and canonical codes
__device__ void build_code(BzShared &S, uint32_t *freq, int n, int max_len, uint8_t *len, uint32_t *code, int lane)
{
	if (lane == 0) S.n_used = 0;
	__syncthreads();
	{
		uint32_t mine = 0;
		for (int s = lane; s < n; s += 64) { len[s] = 0; mine += freq[s] != 0; }
		if (mine) atomicAdd(&S.n_used, mine);
	}
	__syncthreads();
	if (lane == 0)
		for (int s = 0; S.n_used < 2; ++s)
			if (!freq[s]) { freq[s] = 1; ++S.n_used; }
	__syncthreads();
	for (int s = lane; s < n; s += 64) {
		const uint32_t f = freq[s];
		if (!f) continue;
		const uint32_t key = f << 9 | (uint32_t)s;
		int rank = 0;
		for (int t = 0; t < n; ++t) {
			const uint32_t ft = freq[t];
			rank += ft != 0 && (ft << 9 | (uint32_t)t) < key;
		}
		S.sorted[rank] = key;
	}
	__syncthreads();
	if (lane == 0) {
		dfl::huff_lengths(S.sorted, (int)S.n_used, max_len, S.work, S.num, len);
		// first code of every length (RFC 1951 3.2.2) into num[]
		uint32_t c = 0, prev = 0;
		for (int l = 1; l <= max_len; ++l) {
			c = (c + prev) << 1;
			prev = S.num[l];
			S.num[l] = c;
		}
	}
	__syncthreads();
	for (int s = lane; s < n; s += 64) {
		const uint32_t l = len[s];
		uint32_t c = 0;
		if (l) {
			uint32_t before = 0;
			for (int t = 0; t < s; ++t) before += len[t] == l;
			c = (__brev(S.num[l] + before) >> (32 - l)) | l << 16;
		}
		code[s] = c;
	}
	__syncthreads();
}

__global__ __launch_bounds__(64) void bgzf_deflate_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ cut, int n_blocks,
                                                          uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes, uint16_t *__restrict__ tokens,
                                                          unsigned long long *__restrict__ meta, const uint32_t *__restrict__ n_dev)
{
	__shared__ BzShared S;
	const int lane = (int)threadIdx.x;
	if (n_dev) n_blocks = (int)*n_dev;   // (the BAM stage: the cuts were made on the device, bam_kernel.hip)
	uint16_t *const tok = tokens + (size_t)blockIdx.x * BGZF_DEV_INPUT;
	if (lane < 32) {
		uint32_t p = 0x40000000u;   // x^1
		for (int k = 0; k < lane; ++k) p = dfl::gf_mul(p, p);
		S.x2n[lane] = p;
	}
	__syncthreads();
	for (int b = (int)blockIdx.x; b < n_blocks; b += (int)gridDim.x) {
		const uint8_t *const in = text + cut[b];
		const uint32_t n = cut[b + 1] - cut[b];   // 1 .. BGZF_DEV_INPUT
		uint8_t *const slot = slots + (size_t)b * BZ_SLOT;
		uint32_t *const slot32 = (uint32_t *)slot;

		for (int i = lane; i < BZ_HASH_SIZE; i += 64) S.table[i] = 0;
		for (int i = lane; i < 288; i += 64) S.freq_ll[i] = 0;
		if (lane < 32) { S.freq_d[lane] = 0; S.freq_cl[lane] = 0; }
		S.stage[lane] = 0;
		if (lane == 0) { S.bits = 0; S.crc = 0; }
		__syncthreads();

		// ---- 1. CRC32 ----
		{
			const uint32_t nd = n >> 2;
			const uint32_t x2048 = S.x2n[11];
			uint32_t acc = 0, last = 0;
			bool any = false;
			for (uint32_t k = (uint32_t)lane; k < nd; k += 64) { acc = dfl::gf_mul(acc, x2048) ^ ld32(in + 4 * k); last = k; any = true; }
			uint32_t part = any ? dfl::gf_mul(acc, dfl::gf_xpow(S.x2n, 32u + 8u * (n - 4 * last - 4))) : 0u;
			const uint32_t tb = n & 3u;
			if (lane == 0 && tb) {
				uint32_t t = 0;
				for (uint32_t k = 0; k < tb; ++k) t |= (uint32_t)in[4 * nd + k] << (8 * k);
				part ^= dfl::gf_mul(t, dfl::gf_xpow(S.x2n, 8u * tb));
			}
			atomicXor(&S.crc, part);
		}

		// ---- 2. matching ----
		uint32_t n_tok = 0, carry = 0;   // token words so far; positions of the next window that the last match covers
		for (uint32_t base = 0; base < n; base += 64) {
			const uint32_t p = base + (uint32_t)lane, cnt = n - base < 64 ? n - base : 64;
			const bool valid = p < n, have = p + 4 <= n;
			const uint32_t w = valid ? ld32(in + p) : 0u;
			const uint32_t h = (w * 2654435761u) >> (32 - BZ_HASH_BITS);
			const uint32_t cand1 = have ? S.table[h] : 0u;
			__syncthreads();
			if (have) atomicMax(&S.table[h], p + 1);
			uint32_t mlen = 0, dist = 0;
			if (carry < cnt && cand1) {
				const uint32_t c = cand1 - 1;
				dist = p - c;
				if (dist <= BZ_MAX_DIST) {
					const uint32_t maxl = n - p < BZ_MAX_MATCH ? n - p : BZ_MAX_MATCH;
					uint32_t k = 0;
					while (k < maxl) {
						const uint32_t x = ld32(in + p + k) ^ ld32(in + c + k);
						if (x) { k += (uint32_t)__builtin_ctz(x) >> 3; break; }
						k += 4;
					}
					if (k > maxl) k = maxl;
					mlen = k >= BZ_MIN_MATCH ? k : 0u;
				}
			}
			S.wlen[lane] = mlen;
			__syncthreads();
			// the window's tokens: a scalar walk (every lane computes the same)
			const uint64_t M = __ballot(mlen != 0);
			uint64_t sel = 0;
			uint32_t cur = carry;
			while (cur < cnt) {
				const uint64_t rest = M >> cur;
				if (!rest) { sel |= lowmask(cnt - cur) << cur; cur = cnt; break; }
				const uint32_t skip = (uint32_t)__builtin_ctzll(rest);
				sel |= lowmask(skip) << cur;
				cur += skip;
				sel |= 1ull << cur;
				cur += (uint32_t)__builtin_amdgcn_readfirstlane((int)S.wlen[cur]);
			}
			carry = cur - cnt;
			const uint64_t below = lowmask((uint32_t)lane), SM = sel & M;
			if ((sel >> lane) & 1) {
				const uint32_t at = n_tok + (uint32_t)__popcll(sel & below) + (uint32_t)__popcll(SM & below);
				if (mlen) {
					uint32_t lc, lnb, lex, dc, dnb, dex;
					dfl::len_symbol(mlen, lc, lnb, lex);
					dfl::dist_symbol(dist, dc, dnb, dex);
					tok[at] = (uint16_t)(0x4000u | (mlen - 3));
					tok[at + 1] = (uint16_t)(0x8000u | (dist - 1));
					atomicAdd(&S.freq_ll[lc], 1u);
					atomicAdd(&S.freq_d[dc], 1u);
					atomicAdd(&S.bits, lnb + dnb);
				} else {
					tok[at] = (uint16_t)(w & 0xffu);
					atomicAdd(&S.freq_ll[w & 0xffu], 1u);
				}
			}
			n_tok += (uint32_t)__popcll(sel) + (uint32_t)__popcll(SM);
			__syncthreads();
		}
		if (lane == 0) S.freq_ll[256] = 1;
		__syncthreads();

		// ---- 3. codes ----
		build_code(S, S.freq_ll, BZ_NLL, 15, S.len_ll, S.code_ll, lane);
		build_code(S, S.freq_d, BZ_ND, 15, S.len_d, S.code_d, lane);
		for (int k = lane; k < BZ_NLL + BZ_ND; k += 64) atomicAdd(&S.freq_cl[k < BZ_NLL ? S.len_ll[k] : S.len_d[k - BZ_NLL]], 1u);
		__syncthreads();
		build_code(S, S.freq_cl, BZ_NCL, 7, S.len_cl, S.code_cl, lane);

		// ---- 4. the size of the coded form (symbols added to make a code complete are counted although never sent: an upper bound) ----
		{
			uint32_t mine = 0;
			for (int s = lane; s < BZ_NLL; s += 64) mine += S.freq_ll[s] * S.len_ll[s];
			if (lane < BZ_ND) mine += S.freq_d[lane] * S.len_d[lane];
			if (lane < BZ_NCL) mine += S.freq_cl[lane] * S.len_cl[lane];
			if (lane == 0) mine += 3 + 14 + 3 * BZ_NCL;
			atomicAdd(&S.bits, mine);
		}
		__syncthreads();
		const uint32_t coded_bytes = ((uint32_t)__builtin_amdgcn_readfirstlane((int)S.bits) + 7) >> 3, crc = dfl::crc_finish(S.x2n, S.crc, n);
		const bool stored = coded_bytes >= n + 5 || coded_bytes > BZ_SLOT - BZ_HEAD - BZ_TAIL;   // (uniform)
		__syncthreads();

		if (lane < 4) slot32[lane] = lane == 0 ? 0x04088b1fu : lane == 1 ? 0u : lane == 2 ? 0x0006ff00u : 0x00024342u;   // 1f 8b 08 04 | mtime | xfl 00, os ff, xlen 06 00 | 'B' 'C' 02 00
		uint32_t end;   // bytes of the block before the trailer
		if (stored) {
			if (lane == 0) {
				slot[18] = 1;                 // BFINAL, BTYPE 00
				slot[19] = (uint8_t)n; slot[20] = (uint8_t)(n >> 8);
				slot[21] = (uint8_t)~n; slot[22] = (uint8_t)(~n >> 8);
			}
			for (uint32_t k = (uint32_t)lane; k < n; k += 64) slot[23 + k] = in[k];
			end = 23 + n;
		} else {
			uint32_t pos = 8 * BZ_HEAD;   // the stream starts in the upper half of dword 4; its lower half (BSIZE) is written at the end
			emit(S, slot32, pos, 5u | (BZ_NLL - 257) << 3 | (BZ_ND - 1) << 8 | (BZ_NCL - 4) << 13, lane == 0 ? 17u : 0u, lane);
			{
				const uint32_t order = lane < 3 ? 16u + (uint32_t)lane : lane == 3 ? 0u : (lane & 1) ? 8u - (uint32_t)(lane - 3) / 2 : 8u + (uint32_t)(lane - 4) / 2;
				// 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: lane 4 -> 8, 5 -> 7, 6 -> 9, 7 -> 6, ...
				emit(S, slot32, pos, lane < BZ_NCL ? S.len_cl[order] : 0u, lane < BZ_NCL ? 3u : 0u, lane);
			}
			for (int k0 = 0; k0 < BZ_NLL + BZ_ND; k0 += 64) {
				const int k = k0 + lane;
				uint32_t c = 0;
				if (k < BZ_NLL + BZ_ND) c = S.code_cl[k < BZ_NLL ? S.len_ll[k] : S.len_d[k - BZ_NLL]];
				emit(S, slot32, pos, c & 0xffffu, c >> 16, lane);
			}
			for (uint32_t j0 = 0; j0 < n_tok; j0 += 64) {
				const uint32_t j = j0 + (uint32_t)lane;
				uint32_t val = 0, nb = 0;
				if (j < n_tok) {
					const uint32_t t = tok[j];
					uint32_t c, enb = 0, ex = 0, sym;
					if (t & 0x8000u) { dfl::dist_symbol((t & 0x7fffu) + 1, sym, enb, ex); c = S.code_d[sym]; }
					else if (t & 0x4000u) { dfl::len_symbol((t & 0x3fffu) + 3, sym, enb, ex); c = S.code_ll[sym]; }
					else c = S.code_ll[t];
					val = (c & 0xffffu) | ex << (c >> 16);
					nb = (c >> 16) + enb;
				}
				emit(S, slot32, pos, val, nb, lane);
			}
			emit(S, slot32, pos, S.code_ll[256] & 0xffffu, lane == 0 ? S.code_ll[256] >> 16 : 0u, lane);
			if (lane == 0 && (pos & 31u)) slot32[pos >> 5] = S.stage[0];   // the last, partly filled dword
			end = (pos + 7) >> 3;
		}
		// the trailer and BSIZE overwrite bytes that the stream's dwords have covered: behind them
		__threadfence();
		__syncthreads();
		if (lane == 0) {
			const uint32_t total = end + BZ_TAIL;
			slot[16] = (uint8_t)((total - 1) & 0xff); slot[17] = (uint8_t)((total - 1) >> 8);
			for (int k = 0; k < 4; ++k) { slot[end + k] = (uint8_t)(crc >> (8 * k)); slot[end + 4 + k] = (uint8_t)(n >> (8 * k)); }
			sizes[b] = total;
			if (stored) atomicAdd(&meta[1], 1ull);
		}
		__syncthreads();
	}
}

// block b's bytes from its slot to their place in the packed stream: behind the blocks before it
__global__ __launch_bounds__(256) void bgzf_gather_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes, int n_blocks,
                                                          uint8_t *__restrict__ out, unsigned long long *__restrict__ meta, const uint32_t *__restrict__ n_dev)
{
	__shared__ unsigned long long off;
	const int b = (int)blockIdx.x;
	if (n_dev) n_blocks = (int)*n_dev;
	if (b >= n_blocks) return;
	if (threadIdx.x == 0) off = 0;
	__syncthreads();
	unsigned long long mine = 0;
	for (int i = (int)threadIdx.x; i < b; i += (int)blockDim.x) mine += sizes[i];
	if (mine) atomicAdd(&off, mine);
	__syncthreads();
	const unsigned long long at = off;
	const uint32_t n = sizes[b];
	const uint8_t *src = slots + (size_t)b * BZ_SLOT;
	for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) out[at + k] = src[k];
	if (b == n_blocks - 1 && threadIdx.x == 0) meta[0] = at + n;
}

} // namespace

void launch_bgzf_deflate(void *stream, const uint8_t *d_text, const uint32_t *d_cut, int n_blocks, uint8_t *d_slots, uint32_t *d_sizes,
                         uint16_t *d_tokens, int grid, unsigned long long *d_meta, const uint32_t *d_n_blocks)
{
	if (n_blocks <= 0) return;
	if (grid > n_blocks) grid = n_blocks;
	hipLaunchKernelGGL(bgzf_deflate_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, d_text, d_cut, n_blocks, d_slots, d_sizes, d_tokens, d_meta,
	                   d_n_blocks);
	HIP_OK(hipGetLastError());
}

void launch_bgzf_gather(void *stream, const uint8_t *d_slots, const uint32_t *d_sizes, int n_blocks, uint8_t *d_out, unsigned long long *d_meta,
                        const uint32_t *d_n_blocks)
{
	if (n_blocks <= 0) return;
	hipLaunchKernelGGL(bgzf_gather_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, d_slots, d_sizes, n_blocks, d_out, d_meta, d_n_blocks);
	HIP_OK(hipGetLastError());
}

} // namespace mbw
