// bgzf_stage.hip — mi355x_bgzf_compress_dev: SAM text to BGZF blocks through the device encoder (bgzf_kernel.hip), with the contract of
// mi355x_bgzf_compress (sampost.cpp) and its cuts.  DESIGN §8.2.
//
// A call leases a context from a small pool and takes the text through it in pieces of at most BZ_PIECE blocks (33 MB), two pieces
// in flight, each on a stream of its own: while the kernels of one piece run, the host copies the next piece's text into page-locked
// memory and its upload runs beside them.  Per piece: text and cuts up, bgzf_deflate_kernel (a block per wavefront into 64-KiB slots),
// bgzf_gather_kernel (the slots closed up), the packed size back, then only the compressed bytes back.  The caller's text and out are
// pageable, so both ends go through the context's page-locked buffers.  A context's buffers have one size whatever the text: after its
// first call a context never allocates again (mi355x_buffer_growths stands still).
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <vector>
#include "hip_util.h"
#include "device.h"

namespace mbw {
namespace {

constexpr int BZ_CTX = 8;                 // calls side by side (the driver runs six workers); more callers wait their turn
constexpr int BZ_PIECE = 512;             // blocks per piece = workgroups per launch
constexpr size_t BZ_SLOT_BYTES = 0x10000;
constexpr size_t BZ_TEXT_BYTES = (size_t)BZ_PIECE * BGZF_DEV_INPUT, BZ_TEXT_SLACK = 16;

struct BgzfCtx {
	bool busy = false, ready = false;
	hipStream_t st[2] = {nullptr, nullptr};
	hipEvent_t ev[2] = {nullptr, nullptr};
	DevBuf d_text[2], d_cut[2], d_slots[2], d_sizes[2], d_out[2], d_meta[2], d_tokens[2];
	PinBuf h_text[2], h_cut[2], h_out[2], h_meta[2];
	void init()
	{
		for (int s = 0; s < 2; ++s) {
			HIP_OK(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
			HIP_OK(hipEventCreateWithFlags(&ev[s], hipEventDisableTiming));
			d_text[s].ensure(BZ_TEXT_BYTES + BZ_TEXT_SLACK);
			d_cut[s].ensure(sizeof(uint32_t) * (BZ_PIECE + 1));
			d_slots[s].ensure(BZ_PIECE * BZ_SLOT_BYTES);
			d_sizes[s].ensure(sizeof(uint32_t) * BZ_PIECE);
			d_out[s].ensure(BZ_PIECE * BZ_SLOT_BYTES);
			d_meta[s].ensure(2 * sizeof(unsigned long long));
			h_text[s].ensure(BZ_TEXT_BYTES);
			h_cut[s].ensure(sizeof(uint32_t) * (BZ_PIECE + 1));
			h_out[s].ensure(BZ_PIECE * BZ_SLOT_BYTES);
			h_meta[s].ensure(2 * sizeof(unsigned long long));
			d_tokens[s].ensure(sizeof(uint16_t) * BZ_TEXT_BYTES);   // (per stream: the two pieces' kernels may run side by side)
		}
		ready = true;
	}
	void release()
	{
		for (int s = 0; s < 2; ++s) {
			for (DevBuf *b : {&d_text[s], &d_cut[s], &d_slots[s], &d_sizes[s], &d_out[s], &d_meta[s], &d_tokens[s]}) b->release();
			for (PinBuf *b : {&h_text[s], &h_cut[s], &h_out[s], &h_meta[s]}) b->release();
			if (st[s]) (void)hipStreamDestroy(st[s]);
			if (ev[s]) (void)hipEventDestroy(ev[s]);
			st[s] = nullptr; ev[s] = nullptr;
		}
		ready = false;
	}
};

BgzfCtx g_bz[BZ_CTX];
std::mutex g_bz_mu;
std::condition_variable g_bz_cv;
std::atomic<uint64_t> g_bz_counts[4];   // blocks, stored blocks, bytes in, bytes out

struct BgzfLease {
	BgzfCtx *c = nullptr;
	BgzfLease()
	{
		std::unique_lock<std::mutex> lk(g_bz_mu);
		for (;;) {
			for (int pass = 0; pass < 2 && !c; ++pass)   // one that has its buffers first
				for (int i = 0; i < BZ_CTX && !c; ++i)
					if (!g_bz[i].busy && (pass == 1 || g_bz[i].ready)) c = &g_bz[i];
			if (c) break;
			g_bz_cv.wait(lk);
		}
		c->busy = true;
		lk.unlock();
		if (!c->ready) c->init();
	}
	~BgzfLease()
	{
		{
			std::lock_guard<std::mutex> lk(g_bz_mu);
			c->busy = false;
		}
		g_bz_cv.notify_one();
	}
};

} // namespace

void release_bgzf_contexts()
{
	std::unique_lock<std::mutex> lk(g_bz_mu);
	for (int i = 0; i < BZ_CTX; ++i) {
		BgzfCtx &x = g_bz[i];
		if (x.busy || !x.ready) continue;
		x.busy = true;   // nobody leases it while its buffers go
		lk.unlock();
		x.release();
		lk.lock();
		x.busy = false;
	}
	g_bz_cv.notify_all();
}

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
	if (n_blocks * BZ_SLOT_BYTES > cap) return 0;
	use_device();
	BgzfLease lease;
	BgzfCtx &C = *lease.c;
	const size_t n_pieces = (n_blocks + BZ_PIECE - 1) / BZ_PIECE;
	auto start = [&](size_t piece) {   // everything of a piece up to its packed size, queued on the piece's stream
		const int s = (int)(piece & 1);
		const size_t b0 = piece * BZ_PIECE, b1 = std::min(n_blocks, b0 + BZ_PIECE), bytes = cut[b1] - cut[b0];
		const int nb = (int)(b1 - b0);
		memcpy(C.h_text[s].p, text + cut[b0], bytes);
		uint32_t *hc = (uint32_t *)C.h_cut[s].p;
		for (int k = 0; k <= nb; ++k) hc[k] = (uint32_t)(cut[b0 + k] - cut[b0]);
		HIP_OK(hipMemcpyAsync(C.d_text[s].p, C.h_text[s].p, bytes, hipMemcpyHostToDevice, C.st[s]));
		HIP_OK(hipMemcpyAsync(C.d_cut[s].p, hc, sizeof(uint32_t) * (nb + 1), hipMemcpyHostToDevice, C.st[s]));
		HIP_OK(hipMemsetAsync(C.d_meta[s].p, 0, 2 * sizeof(unsigned long long), C.st[s]));
		launch_bgzf_deflate(C.st[s], (const uint8_t *)C.d_text[s].p, (const uint32_t *)C.d_cut[s].p, nb, (uint8_t *)C.d_slots[s].p, (uint32_t *)C.d_sizes[s].p,
		                    (uint16_t *)C.d_tokens[s].p, BZ_PIECE, (unsigned long long *)C.d_meta[s].p);
		launch_bgzf_gather(C.st[s], (const uint8_t *)C.d_slots[s].p, (const uint32_t *)C.d_sizes[s].p, nb, (uint8_t *)C.d_out[s].p, (unsigned long long *)C.d_meta[s].p);
		HIP_OK(hipMemcpyAsync(C.h_meta[s].p, C.d_meta[s].p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, C.st[s]));
		HIP_OK(hipEventRecord(C.ev[s], C.st[s]));
	};
	size_t w = 0;
	uint64_t n_stored = 0;
	start(0);
	for (size_t piece = 0; piece < n_pieces; ++piece) {
		const int s = (int)(piece & 1);
		HIP_OK(hipEventSynchronize(C.ev[s]));
		const unsigned long long *hm = (const unsigned long long *)C.h_meta[s].p;
		const size_t bytes = (size_t)hm[0];
		n_stored += hm[1];
		if (w + bytes > cap) die("mi355x_bgzf_compress_dev: %zu bytes of blocks do not fit the %zu the caller gave", w + bytes, cap);
		HIP_OK(hipMemcpyAsync(C.h_out[s].p, C.d_out[s].p, bytes, hipMemcpyDeviceToHost, C.st[s]));
		if (piece + 1 < n_pieces) start(piece + 1);   // (the other stream: its copies and kernels run beside this piece's way back)
		HIP_OK(hipStreamSynchronize(C.st[s]));
		memcpy(out + w, C.h_out[s].p, bytes);
		w += bytes;
	}
	g_bz_counts[0] += n_blocks; g_bz_counts[1] += n_stored; g_bz_counts[2] += len; g_bz_counts[3] += w;
	return w;
}

// what the device path has done since the library was loaded, all callers: blocks, blocks written stored, bytes of text, bytes of blocks
extern "C" void mi355x_bgzf_dev_counts(uint64_t out[4])
{
	for (int k = 0; k < 4; ++k) out[k] = g_bz_counts[k].load();
}
