// deflate_util.h — the arithmetic of the device deflate (bgzf_kernel.hip) that does not need a wavefront: CRC-32 as polynomial
// arithmetic, the length / distance symbols of RFC 1951, and length-limited Huffman code lengths.  Plain functions for host and
// device, so that the host can check them against zlib without a GPU.
#ifndef MBW_DEFLATE_UTIL_H
#define MBW_DEFLATE_UTIL_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MBW_HD __host__ __device__ inline
#else
#define MBW_HD inline
#endif

namespace mbw {
namespace dfl {

// ---- CRC-32 (polynomial 0xedb88320, reflected: bit 31 of a word is x^0, bit 0 is x^31) ----
// a(x) * b(x) mod p(x); 32 steps whatever the operands
MBW_HD uint32_t gf_mul(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) {
		p ^= (a & (0x80000000u >> i)) ? b : 0u;
		b = (b >> 1) ^ ((b & 1u) ? 0xedb88320u : 0u);
	}
	return p;
}
// x2n[k] = x^(2^k) mod p
MBW_HD void gf_x2n_table(uint32_t x2n[32])
{
	uint32_t p = 0x40000000u;   // x^1
	x2n[0] = p;
	for (int k = 1; k < 32; ++k) x2n[k] = p = gf_mul(p, p);
}
// x^e mod p
MBW_HD uint32_t gf_xpow(const uint32_t x2n[32], uint32_t e)
{
	uint32_t p = 0x80000000u;   // x^0
	for (int k = 0; e; e >>= 1, ++k)
		if (e & 1u) p = gf_mul(p, x2n[k]);
	return p;
}
// The register of a CRC that starts at 0 and is not inverted at the end is linear in the message: for a message M of n bytes read as
// the polynomial m(x) (first byte's bit 0 = highest power), raw(M) = m(x) * x^32 mod p, raw(A || B) = raw(A) * x^(8 |B|) + raw(B), and
// zlib's crc32(M) = raw(M) ^ 0xffffffff * x^(8 n) ^ 0xffffffff (the initial and the final inversion).
MBW_HD uint32_t crc_finish(const uint32_t x2n[32], uint32_t raw, uint32_t n_bytes)
{
	return raw ^ gf_mul(0xffffffffu, gf_xpow(x2n, 8u * n_bytes)) ^ 0xffffffffu;
}

// ---- RFC 1951 symbols ----
// match length 3..258 -> code 257..285, number of extra bits, their value
MBW_HD void len_symbol(uint32_t len, uint32_t &code, uint32_t &nb, uint32_t &extra)
{
	const uint32_t l = len - 3;
	if (l < 8) { code = 257 + l; nb = 0; extra = 0; return; }
	if (l == 255) { code = 285; nb = 0; extra = 0; return; }
	nb = (31u - (uint32_t)__builtin_clz(l)) - 2;
	code = 257 + 4 * (nb + 1) + ((l >> nb) & 3u);
	extra = l & ((1u << nb) - 1);
}
// match distance 1..32768 -> code 0..29
MBW_HD void dist_symbol(uint32_t dist, uint32_t &code, uint32_t &nb, uint32_t &extra)
{
	const uint32_t d = dist - 1;
	if (d < 4) { code = d; nb = 0; extra = 0; return; }
	nb = (31u - (uint32_t)__builtin_clz(d)) - 1;
	code = 2 * (nb + 1) + ((d >> nb) & 1u);
	extra = d & ((1u << nb) - 1);
}
MBW_HD uint32_t len_extra_bits(uint32_t code) { return code < 265 || code == 285 ? 0 : (code - 261) >> 2; }
MBW_HD uint32_t dist_extra_bits(uint32_t code) { return code < 4 ? 0 : (code - 2) >> 1; }

// ---- code lengths ----
// sorted[0 .. n_used): the used symbols as (frequency << 9 | symbol), ascending.  Writes len[symbol] (1 .. max_len) for them; the lengths
// satisfy Kraft's equality.  A: n_used words of scratch, num: 33 words.  n_used >= 2.  The minimum-redundancy lengths are found in
// place (Moffat and Katajainen 1995), lengths beyond max_len are cut to it and the code is made complete again by lengthening the
// cheapest codes (the counts per length are adjusted, then the lengths are dealt out by frequency: the rarest symbols get the longest).
MBW_HD void huff_lengths(const uint32_t *sorted, int n, int max_len, uint32_t *A, uint32_t *num, uint8_t *len)
{
	for (int i = 0; i < n; ++i) A[i] = sorted[i] >> 9;
	if (n == 2) { A[0] = A[1] = 1; }
	else {
		A[0] += A[1];
		int root = 0, leaf = 2, next;
		for (next = 1; next < n - 1; ++next) {
			if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
			if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
		}
		A[n - 2] = 0;
		for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
		int avbl = 1, used = 0, dpth = 0;
		root = n - 2; next = n - 1;
		while (avbl > 0) {
			while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
			while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
			avbl = 2 * used; ++dpth; used = 0;
		}
	}
	for (int i = 0; i <= 32; ++i) num[i] = 0;
	for (int i = 0; i < n; ++i) ++num[(int)A[i] > max_len ? max_len : (int)A[i]];
	uint32_t total = 0;
	for (int i = max_len; i > 0; --i) total += num[i] << (max_len - i);
	while (total != (1u << max_len)) {   // (only after a cut: the sum is then above one)
		--num[max_len];
		for (int i = max_len - 1; i > 0; --i)
			if (num[i]) { --num[i]; num[i + 1] += 2; break; }
		--total;
	}
	int j = n;
	for (int i = 1; i <= max_len; ++i)
		for (uint32_t l = num[i]; l > 0; --l) len[sorted[--j] & 511u] = (uint8_t)i;
}

} // namespace dfl
} // namespace mbw
#endif
