// bgzf_in_stage.hip — mi355x_bgzf_inflate_dev: BGZF blocks to their text through the device decoder (bgzf_inflate_kernel.hip), with the
// contract and the results of mi355x_bgzf_inflate (sampost.cpp), which block is reported for malformed input included.  DESIGN §8.3.
//
// The stage is bgzf_stage.hip's the other way round: a call leases a context from a small pool and takes the blocks through it in
// pieces of at most BI_PIECE blocks, two pieces in flight, each on a stream of its own.  Per piece: the compressed bytes and the two
// offset tables up, bgzf_inflate_kernel (a block per wavefront), the text and the status words back.  Two things are simpler than on the
// way out: the text offsets are known from the trailers before the launch, so every block writes to its final place (no gather kernel),
// and only compressed bytes go up.  The caller's buffers are pageable, so both ends of every copy are the context's page-locked buffers.
// A context's buffers have one size whatever the input: after its first call a context never allocates again.
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <vector>
#include "hip_util.h"
#include "device.h"
#include "inflate_util.h"

namespace mbw {
namespace {

constexpr int BI_CTX = 8;                 // calls side by side; more callers wait their turn
constexpr int BI_PIECE = 512;             // blocks per piece = workgroups per launch
constexpr size_t BI_BYTES = (size_t)BI_PIECE * 0x10000;   // a piece's blocks, and a piece's text, at their largest

struct BgzfInCtx {
	bool busy = false, ready = false;
	hipStream_t st[2] = {nullptr, nullptr};
	DevBuf d_comp[2], d_text[2], d_off[2], d_status[2];
	PinBuf h_comp[2], h_text[2], h_off[2], h_status[2];
	void init()
	{
		for (int s = 0; s < 2; ++s) {
			HIP_OK(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
			d_comp[s].ensure(BI_BYTES);
			d_text[s].ensure(BI_BYTES);
			d_off[s].ensure(sizeof(uint32_t) * 2 * (BI_PIECE + 1));
			d_status[s].ensure(sizeof(uint32_t) * BI_PIECE);
			h_comp[s].ensure(BI_BYTES);
			h_text[s].ensure(BI_BYTES);
			h_off[s].ensure(sizeof(uint32_t) * 2 * (BI_PIECE + 1));
			h_status[s].ensure(sizeof(uint32_t) * BI_PIECE);
		}
		ready = true;
	}
	void release()
	{
		for (int s = 0; s < 2; ++s) {
			for (DevBuf *b : {&d_comp[s], &d_text[s], &d_off[s], &d_status[s]}) b->release();
			for (PinBuf *b : {&h_comp[s], &h_text[s], &h_off[s], &h_status[s]}) b->release();
			if (st[s]) (void)hipStreamDestroy(st[s]);
			st[s] = nullptr;
		}
		ready = false;
	}
};

BgzfInCtx g_bi[BI_CTX];
std::mutex g_bi_mu;
std::condition_variable g_bi_cv;
std::atomic<uint64_t> g_bi_counts[4];   // blocks, blocks that failed, compressed bytes, text bytes

struct BgzfInLease {
	BgzfInCtx *c = nullptr;
	BgzfInLease()
	{
		std::unique_lock<std::mutex> lk(g_bi_mu);
		for (;;) {
			for (int pass = 0; pass < 2 && !c; ++pass)   // one that has its buffers first
				for (int i = 0; i < BI_CTX && !c; ++i)
					if (!g_bi[i].busy && (pass == 1 || g_bi[i].ready)) c = &g_bi[i];
			if (c) break;
			g_bi_cv.wait(lk);
		}
		c->busy = true;
		lk.unlock();
		if (!c->ready) c->init();
	}
	~BgzfInLease()
	{
		{
			std::lock_guard<std::mutex> lk(g_bi_mu);
			c->busy = false;
		}
		g_bi_cv.notify_one();
	}
};

} // namespace

void release_bgzf_in_contexts()
{
	std::unique_lock<std::mutex> lk(g_bi_mu);
	for (int i = 0; i < BI_CTX; ++i) {
		BgzfInCtx &x = g_bi[i];
		if (x.busy || !x.ready) continue;
		x.busy = true;   // nobody leases it while its buffers go
		lk.unlock();
		x.release();
		lk.lock();
		x.busy = false;
	}
	g_bi_cv.notify_all();
}

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
		BgzfInLease lease;
		BgzfInCtx &C = *lease.c;
		const size_t n_pieces = (n_blocks + BI_PIECE - 1) / BI_PIECE;
		auto start = [&](size_t piece) {   // everything of a piece, queued on the piece's stream
			const int s = (int)(piece & 1);
			const size_t b0 = piece * BI_PIECE, b1 = std::min(n_blocks, b0 + BI_PIECE);
			const int nb = (int)(b1 - b0);
			const size_t cbytes = (size_t)(blk[b1] - blk[b0]), tbytes = (size_t)(txt[b1] - txt[b0]);   // (each at most BI_BYTES: a block and its text are at most 64 KiB)
			memcpy(C.h_comp[s].p, in + blk[b0], cbytes);
			uint32_t *ho = (uint32_t *)C.h_off[s].p, *hb = ho, *ht = ho + (BI_PIECE + 1);
			for (int k = 0; k <= nb; ++k) { hb[k] = (uint32_t)(blk[b0 + k] - blk[b0]); ht[k] = (uint32_t)(txt[b0 + k] - txt[b0]); }
			uint32_t *dof = (uint32_t *)C.d_off[s].p;
			HIP_OK(hipMemcpyAsync(C.d_comp[s].p, C.h_comp[s].p, cbytes, hipMemcpyHostToDevice, C.st[s]));
			HIP_OK(hipMemcpyAsync(dof, ho, sizeof(uint32_t) * 2 * (BI_PIECE + 1), hipMemcpyHostToDevice, C.st[s]));
			launch_bgzf_inflate(C.st[s], (const uint8_t *)C.d_comp[s].p, (uint32_t)cbytes, dof, dof + (BI_PIECE + 1), nb, (uint8_t *)C.d_text[s].p, (uint32_t)tbytes,
			                    (uint32_t *)C.d_status[s].p);
			HIP_OK(hipMemcpyAsync(C.h_status[s].p, C.d_status[s].p, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, C.st[s]));
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
