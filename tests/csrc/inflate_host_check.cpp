// inflate_host_check.cpp — bgzf_inflate_kernel's arithmetic (mpibwa_amd/csrc/inflate_util.h) run on the host, lane by lane: the kernel's
// steps in the kernel's order, a loop over the 64 lanes where the kernel has the wavefront and nothing where it has a barrier.
// Input: a file of records (u32 size, then one BGZF block).  Output: a line per block: status, FNV-1a hash of the text written, ISIZE.
// Payload, text and window are heap blocks of their exact sizes: tests/test_inflate_kernel_host.py builds this with the address and
// undefined-behaviour sanitizers where the toolchain has them, which then see any access outside them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "inflate_util.h"

using namespace mbw;

static uint32_t run_block(const uint8_t *blk, uint32_t size, std::vector<uint8_t> &text, uint32_t &n_out)
{
	n_out = 0;
	if (size < 26) return ifl::IF_E_INPUT;
	const uint8_t *t = blk + size - 8;
	const uint32_t crc_want = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
	const uint32_t n = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
	if (n > ifl::IF_MAX_TEXT) return ifl::IF_E_SIZE;
	n_out = n;
	// the payload in a heap block of its exact size, so that a read past its end is seen
	std::vector<uint8_t> in(blk + 18, blk + size - 8);
	text.assign(n, 0xee);
	uint8_t *out = text.data();
	std::vector<uint8_t> win(ifl::IF_WINDOW);
	ifl::Decoder D;
	uint32_t tok[ifl::IF_BATCH], x2n[32], acc[64] = {0};
	dfl::gf_x2n_table(x2n);
	ifl::decoder_init(D, in.data(), (uint32_t)in.size());
	uint32_t pos = 0, flushed = 0, done = 0, status = 0;
	const uint32_t max_calls = 8u * (uint32_t)in.size() + 2;
	for (uint32_t call = 0; call < max_calls; ++call) {
		uint32_t nt, nb;
		status = ifl::decode_batch(D, pos, n, tok, nt, nb, done);
		if (status) break;
		if (nt > ifl::IF_BATCH) nt = ifl::IF_BATCH;
		if (pos + nb > n) { status = ifl::IF_E_LONG; break; }
		uint32_t at = pos;
		for (uint32_t j = 0; j < nt; ++j) {
			const uint32_t tk = tok[j];
			for (uint32_t lane = 64; lane-- > 0;) {   // (any order of the lanes must do: the highest first here)
				if (tk >> 16) ifl::place_match(win.data(), at, tk, lane);
				else if (lane == 0) win[at & ifl::IF_WMASK] = (uint8_t)tk;
			}
			at += ifl::tok_len(tk);
		}
		pos += nb;
		for (uint32_t r = 0; r < 80 && flushed + ifl::IF_ROW <= pos; ++r) {
			for (uint32_t lane = 0; lane < 64; ++lane) ifl::flush_row(win.data(), flushed, out, lane, x2n[11], acc[lane]);
			flushed += ifl::IF_ROW;
		}
		if (done) break;
	}
	if (!status && !done) status = ifl::IF_E_INPUT;
	if (!status && pos != n) status = ifl::IF_E_SHORT;
	if (!status && flushed + ifl::IF_ROW <= pos) status = ifl::IF_E_LONG;
	if (!status) {
		uint32_t crc = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) crc ^= ifl::flush_tail(win.data(), n, out, lane, x2n, acc[lane]);
		if (dfl::crc_finish(x2n, crc, n) != crc_want) status = ifl::IF_E_CRC;
	}
	return status;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<uint8_t> blk, text;
	for (;;) {
		uint32_t size;
		if (fread(&size, 4, 1, f) != 1) break;
		blk.resize(size);
		if (size && fread(blk.data(), 1, size, f) != size) { fprintf(stderr, "short record\n"); return 2; }
		std::vector<uint8_t> exact(blk);   // (its own allocation of the exact size)
		uint32_t n = 0;
		const uint32_t st = run_block(exact.data(), size, text, n);
		uint32_t h = 2166136261u;
		if (!st) for (uint32_t k = 0; k < n; ++k) h = (h ^ text[k]) * 16777619u;
		printf("%u %08x %u\n", st, st ? 0u : h, n);
	}
	fclose(f);
	return 0;
}
