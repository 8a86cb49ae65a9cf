// bgzf_in_stage.hip — mi355x_bgzf_inflate_dev: BGZF blocks to their text through the device decoder (bgzf_inflate_kernel.hip), with the
// contract and the results of mi355x_bgzf_inflate (sampost.cpp), which block is reported for malformed input included.  DESIGN §8.3.
//
// A call leases a context from a small pool (ctx_pool.h) and takes the blocks through it in pieces of at most BI_PIECE blocks, two pieces
// in flight, each on a stream of its own with an inflate lane of its own (bgzf_lane.h).  Per piece: the compressed bytes and the two
// offset tables up, bgzf_inflate_kernel (a block per wavefront), the text and the status words back.  Two things are simpler than on the
// way out: the text offsets are known from the trailers before the launch, so every block writes to its final place (no gather kernel),
// and only compressed bytes go up.  The caller's buffers are pageable, so both ends of every copy are the context's page-locked buffers.
// A context's buffers have one size whatever the input: after its first call a context never allocates again.
#include <atomic>
#include <vector>
#include "bgzf_lane.h"
#include "ctx_pool.h"
#include "inflate_util.h"

namespace mbw {
namespace {

constexpr int BI_CTX = 8;                 // calls side by side; more callers wait their turn
constexpr int BI_PIECE = LANE_BLOCKS;     // blocks per piece

struct BgzfInCtx {
	hipStream_t st[2] = {nullptr, nullptr};
	InflateLane lane[2];
	DevBuf d_text[2], d_status[2];
	PinBuf h_text[2], h_status[2];
	void init()
	{
		for (int s = 0; s < 2; ++s) {
			HIP_OK(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
			lane[s].init();
			d_text[s].ensure(LANE_BYTES); h_text[s].ensure(LANE_BYTES);   // a piece's text at its largest
			d_status[s].ensure(sizeof(uint32_t) * BI_PIECE); h_status[s].ensure(sizeof(uint32_t) * BI_PIECE);
		}
	}
	void release()
	{
		for (int s = 0; s < 2; ++s) {
			lane[s].release(); d_text[s].release(); d_status[s].release(); h_text[s].release(); h_status[s].release();
			if (st[s]) (void)hipStreamDestroy(st[s]);
			st[s] = nullptr;
		}
	}
	void drain() { for (hipStream_t s : st) (void)hipStreamSynchronize(s); }
};

CtxPool<BgzfInCtx, BI_CTX> g_bi;
std::atomic<uint64_t> g_bi_counts[4];   // blocks, blocks that failed, compressed bytes, text bytes

} // namespace

void release_bgzf_in_contexts() { g_bi.release_idle(); }

} // namespace mbw

using namespace mbw;

// mi355x_bgzf_inflate on the device: the same results byte for byte, the offset reported for malformed input included.  Re-entrant: calls
// run side by side, with or without a resident index, also beside mem_process_seqs and mi355x_bgzf_compress_dev calls in flight.  Needs
// a gfx950 device; there is no CPU fallback.
extern "C" int64_t mi355x_bgzf_inflate_dev(const uint8_t *in, size_t len, char *out, size_t cap)
{
	std::vector<int64_t> blk, txt;
	const int64_t bad = bgzf_in_plan(in, len, blk, txt);
	const size_t n_blocks = blk.size() - 1;
	if ((uint64_t)txt[n_blocks] > cap) return 0;
	int64_t first_bad = -1;
	uint64_t n_failed = 0;
	if (n_blocks) {
		use_device();
		CtxPool<BgzfInCtx, BI_CTX>::Lease lease(g_bi);
		BgzfInCtx &C = *lease;
		const size_t n_pieces = (n_blocks + BI_PIECE - 1) / BI_PIECE;
		auto start = [&](size_t piece) {   // everything of a piece, queued on the piece's stream (which has done with the piece before last)
			const int s = (int)(piece & 1);
			const size_t b0 = piece * BI_PIECE, b1 = std::min(n_blocks, b0 + BI_PIECE), tbytes = (size_t)(txt[b1] - txt[b0]);
			C.lane[s].queue(C.st[s], in, blk.data(), txt.data(), b0, b1, (uint8_t *)C.d_text[s].p, (uint32_t *)C.d_status[s].p);
			HIP_OK(hipMemcpyAsync(C.h_status[s].p, C.d_status[s].p, sizeof(uint32_t) * (b1 - b0), hipMemcpyDeviceToHost, C.st[s]));
			if (tbytes) HIP_OK(hipMemcpyAsync(C.h_text[s].p, C.d_text[s].p, tbytes, hipMemcpyDeviceToHost, C.st[s]));
		};
		start(0);
		for (size_t piece = 0; piece < n_pieces; ++piece) {
			const int s = (int)(piece & 1);
			if (piece + 1 < n_pieces) start(piece + 1);   // (the other stream: its copies and kernel run beside this piece's way back)
			HIP_OK(hipStreamSynchronize(C.st[s]));
			const size_t b0 = piece * BI_PIECE, b1 = std::min(n_blocks, b0 + BI_PIECE);
			memcpy(out + txt[b0], C.h_text[s].p, (size_t)(txt[b1] - txt[b0]));
			const uint32_t *hs = (const uint32_t *)C.h_status[s].p;
			for (size_t b = b0; b < b1; ++b)
				if (hs[b - b0]) { ++n_failed; if (first_bad < 0) first_bad = blk[b]; }
		}
	}
	g_bi_counts[0] += n_blocks; g_bi_counts[1] += n_failed; g_bi_counts[2] += (uint64_t)blk[n_blocks]; g_bi_counts[3] += (uint64_t)txt[n_blocks];
	if (first_bad >= 0) return -first_bad - 1;
	if (bad >= 0) return -bad - 1;
	return txt[n_blocks];
}

// what the device path has done since the library was loaded, all callers: blocks, blocks that failed, compressed bytes, text bytes
extern "C" void mi355x_bgzf_inflate_dev_counts(uint64_t out[4])
{
	for (int k = 0; k < 4; ++k) out[k] = g_bi_counts[k].load();
}
