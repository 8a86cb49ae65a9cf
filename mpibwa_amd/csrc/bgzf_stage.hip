// bgzf_stage.hip — mi355x_bgzf_compress_dev: SAM text to BGZF blocks through the device encoder (bgzf_kernel.hip), with the contract of
// mi355x_bgzf_compress (sampost.cpp) and its cuts.  DESIGN §8.2.
//
// A call leases a context from a small pool (ctx_pool.h) and takes the text through it in pieces of at most BZ_PIECE blocks (33 MB), two
// pieces in flight, each on a stream of its own with a deflate lane of its own (bgzf_lane.h): while the kernels of one piece run, the host copies the next piece's text into page-locked
// memory and its upload runs beside them.  Per piece: text and cuts up, bgzf_deflate_kernel (a block per wavefront into 64-KiB slots),
// bgzf_gather_kernel (the slots closed up), the packed size back, then only the compressed bytes back.  The caller's text and out are
// pageable, so both ends go through the context's page-locked buffers.  A context's buffers have one size whatever the text: after its
// first call a context never allocates again (mi355x_buffer_growths stands still).
#include <atomic>
#include <vector>
#include "bgzf_lane.h"
#include "ctx_pool.h"

namespace mbw {
namespace {

constexpr int BZ_CTX = 8;                 // calls side by side (the driver runs six workers); more callers wait their turn
constexpr int BZ_PIECE = LANE_BLOCKS;     // blocks per piece

struct BgzfCtx {
	hipStream_t st[2] = {nullptr, nullptr};
	hipEvent_t ev[2] = {nullptr, nullptr};
	DeflateLane lane[2];
	DevBuf d_text[2];
	PinBuf h_text[2];
	void init()
	{
		for (int s = 0; s < 2; ++s) {
			HIP_OK(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
			HIP_OK(hipEventCreateWithFlags(&ev[s], hipEventDisableTiming));
			lane[s].init();
			d_text[s].ensure(LANE_TEXT_BYTES + LANE_SLACK);
			h_text[s].ensure(LANE_TEXT_BYTES);
		}
	}
	void release()
	{
		for (int s = 0; s < 2; ++s) {
			lane[s].release(); d_text[s].release(); h_text[s].release();
			if (st[s]) (void)hipStreamDestroy(st[s]);
			if (ev[s]) (void)hipEventDestroy(ev[s]);
			st[s] = nullptr; ev[s] = nullptr;
		}
	}
	void drain() { for (hipStream_t s : st) (void)hipStreamSynchronize(s); }
};

CtxPool<BgzfCtx, BZ_CTX> g_bz;
std::atomic<uint64_t> g_bz_counts[4];   // blocks, stored blocks, bytes in, bytes out

} // namespace

void release_bgzf_contexts() { g_bz.release_idle(); }

} // namespace mbw

using namespace mbw;

// `len` bytes of SAM text as BGZF blocks into out[cap], compressed on the device: the cuts of mi355x_bgzf_compress, one setting (no
// level).  out needs mi355x_bgzf_bound(len) bytes; returns the compressed size, 0 when cap is too small or len is 0.  Re-entrant: calls
// run side by side, also beside mem_process_seqs calls in flight.  Needs a gfx950 device; there is no CPU fallback.
extern "C" size_t mi355x_bgzf_compress_dev(const char *text, size_t len, uint8_t *out, size_t cap)
{
	if (!len) return 0;
	std::vector<size_t> cut;
	bgzf_cuts(text, len, cut);
	const size_t n_blocks = cut.size() - 1;
	if (n_blocks * LANE_SLOT_BYTES > cap) return 0;
	use_device();
	CtxPool<BgzfCtx, BZ_CTX>::Lease lease(g_bz);
	BgzfCtx &C = *lease;
	const size_t n_pieces = (n_blocks + BZ_PIECE - 1) / BZ_PIECE;
	auto start = [&](size_t piece) {   // everything of a piece up to its packed size, queued on the piece's stream
		const int s = (int)(piece & 1);
		const size_t b0 = piece * BZ_PIECE, b1 = std::min(n_blocks, b0 + BZ_PIECE), bytes = cut[b1] - cut[b0];
		memcpy(C.h_text[s].p, text + cut[b0], bytes);
		HIP_OK(hipMemcpyAsync(C.d_text[s].p, C.h_text[s].p, bytes, hipMemcpyHostToDevice, C.st[s]));
		C.lane[s].cuts_up(C.st[s], cut.data() + b0, (int)(b1 - b0));
		C.lane[s].queue(C.st[s], (const uint8_t *)C.d_text[s].p, (int)(b1 - b0));
		HIP_OK(hipEventRecord(C.ev[s], C.st[s]));
	};
	size_t w = 0;
	uint64_t n_stored = 0;
	start(0);
	for (size_t piece = 0; piece < n_pieces; ++piece) {
		const int s = (int)(piece & 1);
		DeflateLane &L = C.lane[s];
		HIP_OK(hipEventSynchronize(C.ev[s]));
		n_stored += L.stored();
		if (w + L.packed() > cap) die("mi355x_bgzf_compress_dev: %zu bytes of blocks do not fit the %zu the caller gave", w + L.packed(), cap);
		L.fetch(C.st[s]);
		if (piece + 1 < n_pieces) start(piece + 1);   // (the other stream: its copies and kernels run beside this piece's way back)
		HIP_OK(hipStreamSynchronize(C.st[s]));
		w += L.store(out + w);
	}
	g_bz_counts[0] += n_blocks; g_bz_counts[1] += n_stored; g_bz_counts[2] += len; g_bz_counts[3] += w;
	return w;
}

// what the device path has done since the library was loaded, all callers: blocks, blocks written stored, bytes of text, bytes of blocks
extern "C" void mi355x_bgzf_dev_counts(uint64_t out[4])
{
	for (int k = 0; k < 4; ++k) out[k] = g_bz_counts[k].load();
}
