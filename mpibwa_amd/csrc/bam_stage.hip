// bam_stage.hip — mi355x_bam_compress_dev and mi355x_sam_to_bam_dev: a chunk's SAM text to BAM records by the encoder kernels
// (bam_kernel.hip) and on to BGZF blocks by the deflate kernel (bgzf_kernel.hip), with the records and the cuts of mi355x_bam_compress
// (sampost.cpp).  DESIGN §8.4.
//
// The stage is bgzf_stage.hip's with the encoder in front: a call leases a context from a small pool (ctx_pool.h) and takes the text
// through it in pieces of whole lines, at most BAM_DEV_TEXT bytes, two pieces in flight, each on a stream and a deflate lane (bgzf_lane.h)
// of its own.  Per piece: the text up, the line starts, the size pass, the scan, the write pass, the cuts, bgzf_deflate_kernel,
// bgzf_gather_kernel — all queued at once; what comes back is d_meta's two words and the piece's BamDevCtl, then only the compressed
// bytes.  A piece whose ctl says that it is not the device's (a declined line, more lines / bytes / blocks than the buffers hold) is
// encoded by the host encoder, and its records and cuts go up in the encoder's place: the deflate is the device's either way, so the bytes
// of a call do not depend on who encoded.  A malformed line ends the call with the host encoder's code.  A context's buffers have one size
// whatever the text.
#include <atomic>
#include <vector>
#include "bgzf_lane.h"
#include "ctx_pool.h"
#include "bam_util.h"

namespace mbw {
namespace {

constexpr int BM_CTX = 8;
constexpr size_t BM_CONTIG_BYTES = 4u << 20;   // the contig table; a larger one sends the call's pieces to the host encoder

struct BamCtx {
	hipStream_t st[2] = {nullptr, nullptr};
	hipEvent_t ev[2] = {nullptr, nullptr};
	DeflateLane lane[2];   // (the cuts kernel writes the lane's d_cut)
	DevBuf d_text[2], d_chunk[2], d_start[2], d_plan[2], d_group[2], d_off[2], d_next[2], d_bam[2], d_ctl[2], d_contigs;
	PinBuf h_text[2], h_ctl[2], h_ctl0;
	void init()
	{
		d_contigs.ensure(BM_CONTIG_BYTES);
		BamDevCtl *c0 = (BamDevCtl *)h_ctl0.ensure(sizeof(BamDevCtl));
		memset(c0, 0, sizeof *c0);
		c0->err = 0xffffffffu;
		for (int s = 0; s < 2; ++s) {
			HIP_OK(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
			HIP_OK(hipEventCreateWithFlags(&ev[s], hipEventDisableTiming));
			lane[s].init();
			d_text[s].ensure(BAM_DEV_TEXT + LANE_SLACK);
			d_chunk[s].ensure(sizeof(uint32_t) * (BAM_DEV_TEXT / BAM_DEV_CHUNK + 2));
			d_start[s].ensure(sizeof(uint32_t) * (BAM_DEV_LINES + 1));
			d_plan[s].ensure(bam_plan_bytes() * BAM_DEV_LINES);
			d_group[s].ensure(sizeof(uint32_t) * (BAM_DEV_LINES / 64 + 1));
			d_off[s].ensure(sizeof(uint32_t) * (BAM_DEV_LINES + 1));
			d_next[s].ensure(sizeof(uint32_t) * BAM_DEV_LINES);
			d_bam[s].ensure(BAM_DEV_BYTES + LANE_SLACK);
			d_ctl[s].ensure(sizeof(BamDevCtl));
			h_text[s].ensure(BAM_DEV_BYTES + LANE_SLACK);   // a piece's text, or the records the host made of it
			h_ctl[s].ensure(sizeof(BamDevCtl));
		}
	}
	void release()
	{
		d_contigs.release(); h_ctl0.release();
		for (int s = 0; s < 2; ++s) {
			lane[s].release();
			for (DevBuf *b : {&d_text[s], &d_chunk[s], &d_start[s], &d_plan[s], &d_group[s], &d_off[s], &d_next[s], &d_bam[s], &d_ctl[s]}) b->release();
			h_text[s].release(); h_ctl[s].release();
			if (st[s]) (void)hipStreamDestroy(st[s]);
			if (ev[s]) (void)hipEventDestroy(ev[s]);
			st[s] = nullptr; ev[s] = nullptr;
		}
	}
	void drain() { for (hipStream_t s : st) (void)hipStreamSynchronize(s); }   // (a call that ends early leaves nothing queued on the context)
	BamDevBufs bufs(int s, uint32_t text_len) const
	{
		BamDevBufs B;
		B.text = (const uint8_t *)d_text[s].p; B.text_len = text_len; B.contigs = d_contigs.p;
		B.chunk_cnt = (uint32_t *)d_chunk[s].p; B.line_start = (uint32_t *)d_start[s].p; B.plan = d_plan[s].p; B.group = (uint32_t *)d_group[s].p;
		B.rec_off = (uint32_t *)d_off[s].p; B.next = (uint32_t *)d_next[s].p; B.bam = (uint8_t *)d_bam[s].p; B.cut = (uint32_t *)lane[s].d_cut.p;
		B.ctl = (BamDevCtl *)d_ctl[s].p;
		return B;
	}
};

CtxPool<BamCtx, BM_CTX> g_bm;
std::atomic<uint64_t> g_bm_counts[6];   // records, records of pieces the host encoded, SAM bytes, BAM bytes, blocks, compressed bytes

// the text in pieces of whole lines: piece[k] .. piece[k + 1]; a line longer than a piece stands alone (it is the host's)
void bam_pieces(const char *sam, size_t body, std::vector<size_t> &piece)
{
	piece.assign(1, 0);
	for (size_t at = 0; at < body;) {
		size_t hi = body;
		if (body - at > BAM_DEV_TEXT) {
			const void *nl = memrchr(sam + at, '\n', BAM_DEV_TEXT);
			hi = nl ? (size_t)((const char *)nl - sam) + 1 : (size_t)((const char *)memchr(sam + at, '\n', body - at) - sam) + 1;
		}
		piece.push_back(hi);
		at = hi;
	}
}

// Both entry points.  compress: BGZF blocks into out; else the records.
int64_t bam_dev(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap, int64_t *n_records, bool compress)
{
	if (n_records) *n_records = 0;
	const void *last_nl = len ? memrchr(sam, '\n', len) : nullptr;
	const size_t body = last_nl ? (size_t)((const char *)last_nl - sam) + 1 : 0;   // the whole lines
	if (!body) return body < len ? -1 : 0;
	std::vector<uint8_t> blob;
	bam_contig_blob(bns, blob);
	const bam::ContigTable tab = bam::contig_table_at(blob.data());
	std::vector<size_t> piece;
	bam_pieces(sam, body, piece);
	const size_t n_pieces = piece.size() - 1;
	use_device();
	CtxPool<BamCtx, BM_CTX>::Lease lease(g_bm);
	BamCtx &C = *lease;
	const bool table_fits = blob.size() <= BM_CONTIG_BYTES;
	if (table_fits) {
		// (pageable memory: the copy is staged by the runtime and has left blob when the call returns)
		HIP_OK(hipMemcpyAsync(C.d_contigs.p, blob.data(), blob.size(), hipMemcpyHostToDevice, C.st[0]));
		HIP_OK(hipStreamSynchronize(C.st[0]));
	}
	auto start = [&](size_t k) {   // everything of a piece, queued on the piece's stream
		const int s = (int)(k & 1);
		const size_t bytes = piece[k + 1] - piece[k];
		BamDevCtl *hc = (BamDevCtl *)C.h_ctl[s].p;
		if (bytes > BAM_DEV_TEXT || !table_fits) {   // the host's piece before anything runs
			memset(hc, 0, sizeof *hc);
			hc->err = 0xffffffffu; hc->decline = 1;
			HIP_OK(hipEventRecord(C.ev[s], C.st[s]));
			return;
		}
		memcpy(C.h_text[s].p, sam + piece[k], bytes);
		HIP_OK(hipMemcpyAsync(C.d_text[s].p, C.h_text[s].p, bytes, hipMemcpyHostToDevice, C.st[s]));
		HIP_OK(hipMemcpyAsync(C.d_ctl[s].p, C.h_ctl0.p, sizeof(BamDevCtl), hipMemcpyHostToDevice, C.st[s]));
		const BamDevBufs B = C.bufs(s, (uint32_t)bytes);
		launch_bam_encode(C.st[s], B);
		if (compress) {
			launch_bam_cuts(C.st[s], B);
			C.lane[s].queue(C.st[s], B.bam, LANE_BLOCKS, &B.ctl->n_blocks);   // (the cuts and their number stay on the device)
		}
		HIP_OK(hipMemcpyAsync(hc, C.d_ctl[s].p, sizeof(BamDevCtl), hipMemcpyDeviceToHost, C.st[s]));
		HIP_OK(hipEventRecord(C.ev[s], C.st[s]));
	};
	size_t w = 0;
	uint64_t n_rec = 0, n_host_rec = 0, bam_bytes = 0, n_blocks = 0;
	std::vector<uint8_t> recs;
	std::vector<uint64_t> off;
	std::vector<size_t> cut;
	start(0);
	for (size_t k = 0; k < n_pieces; ++k) {
		const int s = (int)(k & 1);
		DeflateLane &L = C.lane[s];
		HIP_OK(hipEventSynchronize(C.ev[s]));
		const BamDevCtl ctl = *(const BamDevCtl *)C.h_ctl[s].p;
		const bool mine = ctl.err == 0xffffffffu && !ctl.decline;
		if (k + 1 < n_pieces && mine) start(k + 1);   // (the other stream: its copies and kernels run beside this piece's way back)
		if (!mine) {
			// the host encoder's records (or its error code, for the whole text's offsets)
			const int64_t total = bam_encode_host(sam + piece[k], piece[k + 1] - piece[k], tab, recs, &off);
			if (total < 0) return total - (int64_t)piece[k];
			const uint64_t nr = off.size() - 1;
			n_rec += nr; n_host_rec += nr; bam_bytes += (uint64_t)total;
			if (!compress) {
				if (w + (size_t)total > cap) return 0;
				memcpy(out + w, recs.data(), (size_t)total);
				w += (size_t)total;
			} else {
				bam_cuts(off, cut);
				// through the deflate kernel in runs of at most BAM_DEV_BLOCKS blocks
				for (size_t b0 = 0; b0 + 1 < cut.size(); b0 += BAM_DEV_BLOCKS) {
					const size_t b1 = std::min(cut.size() - 1, b0 + BAM_DEV_BLOCKS), bytes = cut[b1] - cut[b0];
					memcpy(C.h_text[s].p, recs.data() + cut[b0], bytes);
					HIP_OK(hipMemcpyAsync(C.d_bam[s].p, C.h_text[s].p, bytes, hipMemcpyHostToDevice, C.st[s]));
					L.cuts_up(C.st[s], cut.data() + b0, (int)(b1 - b0));
					L.queue(C.st[s], (const uint8_t *)C.d_bam[s].p, (int)(b1 - b0));
					HIP_OK(hipStreamSynchronize(C.st[s]));
					if (w + L.packed() > cap) return 0;
					L.fetch(C.st[s]);
					HIP_OK(hipStreamSynchronize(C.st[s]));
					w += L.store(out + w); n_blocks += b1 - b0;
				}
			}
			if (k + 1 < n_pieces) start(k + 1);
			continue;
		}
		n_rec += ctl.n_lines; bam_bytes += ctl.bam_bytes;
		if (!compress) {   // the records, through the lane's page-locked bytes
			if (w + ctl.bam_bytes > cap) return 0;
			HIP_OK(hipMemcpyAsync(L.h_out.p, C.d_bam[s].p, ctl.bam_bytes, hipMemcpyDeviceToHost, C.st[s]));
			HIP_OK(hipStreamSynchronize(C.st[s]));
			memcpy(out + w, L.h_out.p, ctl.bam_bytes);
			w += ctl.bam_bytes;
		} else {
			if (w + L.packed() > cap) return 0;
			L.fetch(C.st[s]);
			HIP_OK(hipStreamSynchronize(C.st[s]));
			w += L.store(out + w); n_blocks += ctl.n_blocks;
		}
	}
	if (body < len) return -(int64_t)body - 1;   // a last line without '\n', and no malformed line before it
	if (n_records) *n_records = (int64_t)n_rec;
	g_bm_counts[0] += n_rec; g_bm_counts[1] += n_host_rec; g_bm_counts[2] += len; g_bm_counts[3] += bam_bytes;
	g_bm_counts[4] += n_blocks; g_bm_counts[5] += compress ? w : 0;
	return (int64_t)w;
}

} // namespace

void release_bam_contexts() { g_bm.release_idle(); }

} // namespace mbw

using namespace mbw;

// mi355x_sam_to_bam from the kernels: the same records, the same error codes (include/mpibwa_amd.h)
extern "C" int64_t mi355x_sam_to_bam_dev(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap, int64_t *n_records)
{
	return bam_dev(sam, len, bns, out, cap, n_records, false);
}

// mi355x_bam_compress on the device: the records and the cuts of the host path, the deflate kernel's one setting instead of a level
extern "C" int64_t mi355x_bam_compress_dev(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap)
{
	return bam_dev(sam, len, bns, out, cap, nullptr, true);
}

extern "C" void mi355x_bam_dev_counts(uint64_t out[6])
{
	for (int k = 0; k < 6; ++k) out[k] = g_bm_counts[k].load();
}
