// bgzf_inflate_kernel.hip — BGZF blocks inflated on the device: the counterpart of bgzf_kernel.hip.  DESIGN §8.3.
//
// A workgroup is ONE wavefront and takes ONE block: from its deflate stream in HBM to its text at text + text_off[b], with the text's
// CRC32 compared with the trailer's.  The arithmetic is inflate_util.h's, which the host runs lane by lane against zlib; this file adds
// the barriers between its steps and nothing else.
//
//   1. Lane 0 decodes the stream into a batch of at most 64 tokens (decode_batch: block headers, code tables, symbols, every check of
//      the format).  Decoding is serial by nature; the rate of the kernel is the number of waves in flight (four per CU by LDS).
//   2. The batch's bytes enter a circular window of 32 KiB in LDS in token order: a literal by lane 0, a match by all lanes (64 bytes a
//      step, source index k mod distance).  The order is kept because a later token may overwrite the window slot (position - 32 768)
//      that an earlier match of the batch still reads.  Back-references read LDS only, never text that the wave has just sent to HBM.
//   3. Whole rows of 256 bytes leave the window for HBM (64 consecutive bytes per store instruction: the text's place has no alignment)
//      and enter the CRC: lane i takes dword i of every row by a Horner step in GF(2)[x] / p; the lanes' registers are moved to their
//      places and xor-ed together at the end (deflate_util.h).
//
// Compressed files are user input.  The payload is read through a bit reader that never passes the payload's end, every write to the
// text stands below the ISIZE that sized the text's place, the batch loop is bounded by the payload's bits, and an error is a status
// word per block: after it the wave leaves by the common exit.  Cross-lane operations (readfirstlane) stand in wave-uniform code only.
#include "hip_util.h"
#include "device.h"
#include "inflate_util.h"

namespace mbw {
namespace {

struct IfShared {
	alignas(16) uint8_t win[ifl::IF_WINDOW];
	ifl::Decoder dec;
	uint32_t tok[ifl::IF_BATCH];
	uint32_t x2n[32];
	uint32_t n_tok, n_bytes, done, status, crc;
};

__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t *__restrict__ comp, uint32_t comp_len, const uint32_t *__restrict__ blk_off,
                                                          const uint32_t *__restrict__ text_off, int n_blocks, uint8_t *__restrict__ text, uint32_t text_cap,
                                                          uint32_t *__restrict__ status_out)
{
	__shared__ IfShared S;
	const uint32_t lane = threadIdx.x;
	const int b = (int)blockIdx.x;
	if (b >= n_blocks) return;
	if (lane < 32) {
		uint32_t p = 0x40000000u;   // x^1
		for (uint32_t k = 0; k < lane; ++k) p = dfl::gf_mul(p, p);
		S.x2n[lane] = p;
	}
	const uint32_t o0 = blk_off[b], o1 = blk_off[b + 1], t0 = text_off[b], t1 = text_off[b + 1];
	uint32_t status = ifl::IF_OK;
	// what the host has checked, checked again: nothing below reads or writes outside these
	if (o1 > comp_len || o1 < o0 || o1 - o0 < 26) status = ifl::IF_E_INPUT;
	else if (t1 < t0 || t1 > text_cap || t1 - t0 > ifl::IF_MAX_TEXT) status = ifl::IF_E_SIZE;
	status = uni(status);
	const uint32_t in_len = status ? 0u : o1 - o0 - 26, n = status ? 0u : t1 - t0;
	const uint8_t *const in = comp + (status ? 0u : o0 + 18);
	uint8_t *const out = text + (status ? 0u : t0);
	uint32_t crc_want = 0;
	if (!status) {
		const uint8_t *t = comp + o1 - 8;
		crc_want = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
	}
	if (lane == 0) { ifl::decoder_init(S.dec, in, in_len); S.crc = 0; S.status = 0; S.done = 0; S.n_tok = 0; S.n_bytes = 0; }
	__syncthreads();

	const uint32_t x2048 = S.x2n[11];
	uint32_t pos = 0, flushed = 0, acc = 0, done = 0;
	const uint32_t max_calls = status ? 0u : 8u * in_len + 2;   // (decode_batch: a call consumes a bit, fails or is the last)
	for (uint32_t call = 0; call < max_calls; ++call) {
		if (lane == 0) {
			uint32_t nt, nb, dn;
			const uint32_t st = ifl::decode_batch(S.dec, pos, n, S.tok, nt, nb, dn);
			S.n_tok = nt; S.n_bytes = nb; S.done = dn; S.status = st;
		}
		__syncthreads();
		status = uni(S.status);
		if (status) break;
		const uint32_t nt = min(uni(S.n_tok), ifl::IF_BATCH), nb = uni(S.n_bytes);
		if (pos + nb > n) { status = ifl::IF_E_LONG; break; }   // (decode_batch has checked it token by token)
		uint32_t at = pos;
		for (uint32_t j = 0; j < nt; ++j) {
			const uint32_t t = uni(S.tok[j]);
			if (t >> 16) ifl::place_match(S.win, at, t, lane);
			else if (lane == 0) S.win[at & ifl::IF_WMASK] = (uint8_t)t;
			at += ifl::tok_len(t);
			__syncthreads();
		}
		pos += nb;
		for (uint32_t r = 0; r < 80 && flushed + ifl::IF_ROW <= pos; ++r) {   // (a batch has at most 16 512 bytes: 65 rows)
			ifl::flush_row(S.win, flushed, out, lane, x2048, acc);
			flushed += ifl::IF_ROW;
		}
		done = uni(S.done);
		__syncthreads();
		if (done) break;
	}
	if (!status && !done) status = ifl::IF_E_INPUT;
	if (!status && pos != n) status = ifl::IF_E_SHORT;
	if (!status && flushed + ifl::IF_ROW <= pos) status = ifl::IF_E_LONG;   // (cannot be: the rows loop above has room for a batch)
	if (!status) {
		const uint32_t part = ifl::flush_tail(S.win, n, out, lane, S.x2n, acc);
		atomicXor(&S.crc, part);
	}
	__syncthreads();
	if (!status && dfl::crc_finish(S.x2n, S.crc, n) != crc_want) status = ifl::IF_E_CRC;
	if (lane == 0) status_out[b] = status;
}

} // namespace

void launch_bgzf_inflate(void *stream, const uint8_t *d_comp, uint32_t comp_len, const uint32_t *d_blk_off, const uint32_t *d_text_off, int n_blocks,
                         uint8_t *d_text, uint32_t text_cap, uint32_t *d_status)
{
	if (n_blocks <= 0) return;
	hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)n_blocks), dim3(64), 0, (hipStream_t)stream, d_comp, comp_len, d_blk_off, d_text_off, n_blocks,
	                   d_text, text_cap, d_status);
	HIP_OK(hipGetLastError());
}

} // namespace mbw
