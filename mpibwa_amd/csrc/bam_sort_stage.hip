// bam_sort_stage.hip — mi355x_bam_sort_dev: a finished BAM file to coordinate order on the device, with the record stream, the cuts and
// the return codes of mi355x_bam_sort (bam_sort.cpp).  DESIGN §8.5.
//
// The stages of a call, all queued on the call's two streams:
//   inflate   the file's blocks go up in groups of BS_GROUP (two groups in flight), bgzf_inflate_kernel writes every group to its place in
//             ONE resident buffer of the whole inflated stream (launch_bgzf_inflate's offsets are 32-bit: a group is placed by pointer);
//             the host inflates only the leading blocks, to parse the header;
//   walk      a lane per block counts and validates its chain, a scan, a second pass writes offset, size and key (bam_sort_kernel.hip).
//             A stream whose blocks do not all end on a record boundary is a foreign writer's: the host then inflates on the cores,
//             hops once and uploads offsets, sizes and keys — the same bytes come out, the counts say who walked;
//   sort      hipCUB's stable radix sort of (key, index) over the key's bits, the sorted sizes, their exclusive sum;
//   emit      the sorted sizes come back (4 bytes a record), the host makes bam_cuts' cuts and groups them into pieces of at most
//             BAM_DEV_BLOCKS blocks; per piece, alternating the streams: the record gather kernel, bgzf_deflate_kernel, bgzf_gather_kernel,
//             and only compressed bytes come back.  The header's blocks are pieces like the others, their bytes come from the host.
// The sorted stream is never materialised: device memory is the inflated stream, 40 bytes a record and the two piece contexts.  The
// groups go up through an InflateLane per stream and the pieces out through a DeflateLane per stream (bgzf_lane.h), as in
// bgzf_in_stage.hip and bgzf_stage.hip; the context itself stays outside ctx_pool.h's pool: one sort at a time is another contract.
//
// One sort holds the buffers at a time (a mutex); they only grow, so a second call of the same size allocates nothing.  Before it
// allocates, a call compares what it needs with what hipMemGetInfo reports free (plus what the buffers already hold), less BS_MARGIN for
// the other calls' contexts that may grow meanwhile; MPIBWA_BAM_SORT_MAX_BYTES caps the admitted bytes (the tests' way to a refusal).
// The records' arrays can only be sized after the count pass, so there are two such checks; a refusal returns INT64_MIN and has written
// nothing to out.
//
// The BAI index (bam_index_util.h, bam_index_kernel.hip) lives here too, because it is made of what a sort holds:
//   mi355x_bam_sort_index_dev   the sort above, and between its sort and its emit stage the index stages over d_u, d_off, the order
//             d_idx2, the places d_dst and the output's cuts (8 bytes a block go up); every piece's d_sizes come back beside its
//             bytes, so that the host knows each output block's file offset when it writes the index.  The index stages' 52 bytes a
//             record enter this call's second admission check only; a third one covers the runs and the windows once counted.
//   mi355x_bam_index_dev        load_header, load_inflate and walk_count as the sort does them, the write pass of the walk, then the
//             index stages with the file's own order and blocks.  What the device does not take — blocks that do not end on record
//             boundaries, a malformed, out-of-order or too long record — goes to the host path (bam_index.cpp), which decides the code.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>
#include "bgzf_lane.h"
#include "bam_sort_util.h"
#include "bam_index_util.h"

namespace mbw {
namespace {

constexpr int BS_GROUP = LANE_BLOCKS;                            // blocks per inflate launch
constexpr size_t BS_MARGIN = 256u << 20;
constexpr size_t BS_REC_BYTES = 40;                              // offset 8, size 4, key 8 (later the place in the sorted stream), key' 8, index 4, index' 4, sorted size 4

// the index stages (bam_index_kernel.hip): per record the run key 8, v0 8, ref << 32 | end 8 and its maxima 8, beg 4, mapped 4 and its
// sums 4, the head flag 1, the run's first record 4; per contig four words, n_intv and its sums; per run key 8, key' 8, number 4,
// number' 4 and the chunk 16; per window 8
constexpr size_t IX_REC_BYTES = 52, IX_REF_BYTES = 40, IX_RUN_BYTES = 40, IX_WIN_BYTES = 8;

struct SortCtx {
	bool ready = false;
	hipStream_t st[2] = {nullptr, nullptr};
	hipEvent_t ev[2] = {nullptr, nullptr}, ev_g[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
	// of one size whatever the file: per stream an inflate lane for the groups, and for the pieces their bytes and a deflate lane
	InflateLane in[2];
	DeflateLane lane[2];
	DevBuf d_piece[2], d_flag;
	PinBuf h_flag;
	// grow with the file
	DevBuf d_u, d_text_off, d_status, d_cnt, d_first, d_off, d_size, d_key, d_key2, d_idx, d_idx2, d_ssize, d_tmp;
	PinBuf h_status, h_ssize;
	// the index stages' (BamIndexBufs, device.h), allocated by the first call that indexes (as are the lanes' h_sizes)
	DevBuf x_cut, x_rb, x_v0, x_mx, x_mxs, x_beg, x_map, x_maps, x_head, x_rs, x_nsel, x_stat, x_nintv, x_woff, x_rk, x_rk2, x_ri, x_ri2, x_rbeg, x_rend, x_io;
	std::vector<DevBuf *> own()   // the device buffers outside the lanes
	{
		return {&d_piece[0], &d_piece[1], &d_flag, &d_u, &d_text_off, &d_status, &d_cnt, &d_first, &d_off, &d_size, &d_key, &d_key2, &d_idx, &d_idx2, &d_ssize, &d_tmp,
		        &x_cut, &x_rb, &x_v0, &x_mx, &x_mxs, &x_beg, &x_map, &x_maps, &x_head, &x_rs, &x_nsel, &x_stat, &x_nintv, &x_woff, &x_rk, &x_rk2,
		        &x_ri, &x_ri2, &x_rbeg, &x_rend, &x_io};
	}
	std::vector<DevBuf *> all()
	{
		std::vector<DevBuf *> v = own();
		for (int s = 0; s < 2; ++s) {
			for (DevBuf *b : in[s].dev()) v.push_back(b);
			for (DevBuf *b : lane[s].dev()) v.push_back(b);
		}
		return v;
	}
	static constexpr size_t PIECE_BYTES = LANE_TEXT_BYTES + LANE_SLACK, FLAG_BYTES = 16;
	// what init() allocates on the device: the first admission check counts it
	static constexpr size_t fixed_bytes() { return 2 * (InflateLane::dev_bytes() + DeflateLane::dev_bytes() + PIECE_BYTES) + FLAG_BYTES; }
	size_t held()
	{
		size_t n = 0;
		for (DevBuf *b : all()) n += b->cap;
		return n;
	}
	void init()
	{
		d_flag.ensure(FLAG_BYTES); h_flag.ensure(FLAG_BYTES);
		for (int s = 0; s < 2; ++s) {
			HIP_OK(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
			HIP_OK(hipEventCreateWithFlags(&ev[s], hipEventDisableTiming));
			for (int k = 0; k < 2; ++k) HIP_OK(hipEventCreate(&ev_g[s][k]));
			in[s].init(); lane[s].init();
			d_piece[s].ensure(PIECE_BYTES);
		}
		ready = true;
	}
	void release()
	{
		for (DevBuf *b : own()) b->release();
		for (PinBuf *b : {&h_flag, &h_status, &h_ssize}) b->release();
		for (int s = 0; s < 2; ++s) {
			in[s].release(); lane[s].release();
			if (st[s]) (void)hipStreamDestroy(st[s]);
			if (ev[s]) (void)hipEventDestroy(ev[s]);
			for (int k = 0; k < 2; ++k) { if (ev_g[s][k]) (void)hipEventDestroy(ev_g[s][k]); ev_g[s][k] = nullptr; }
			st[s] = nullptr; ev[s] = nullptr;
		}
		ready = false;
	}
};

SortCtx g_bs;
std::mutex g_bs_mu;                       // one sort at a time holds g_bs
std::atomic<uint64_t> g_bs_counts[8];     // calls, records, calls whose walk the host did, inflated bytes, input blocks, output blocks, compressed bytes out, calls refused for memory
std::mutex g_bs_ms_mu;
double g_bs_ms[8];                        // the last call: inflate, walk, sort, emit, all of it (wall ms); the gather kernels (event ms), their bytes; 0
std::atomic<uint64_t> g_bs_refused_need;  // the bytes (margin included) that the last refused call needed

double ms_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// does a call that needs `need` bytes of device memory in g_bs's buffers fit?  (a refusal is counted and its need kept for the caller's message)
std::atomic<uint64_t> g_ix_counts[8];     // calls, records, calls whose walk the host did, runs before the join, chunks written, linear windows, BAI bytes, calls refused for memory
std::mutex g_ix_ms_mu;
double g_ix_ms[8];                        // the last call: inflate, walk, index, serialisation, all of it (wall ms); the index kernels (event ms); 0; 0

bool admitted(size_t need, std::atomic<uint64_t> *counts = g_bs_counts)
{
	size_t free_b = 0, total_b = 0;
	HIP_OK(hipMemGetInfo(&free_b, &total_b));
	size_t have = free_b + g_bs.held();
	if (const char *e = getenv("MPIBWA_BAM_SORT_MAX_BYTES")) have = std::min<size_t>(have, (size_t)strtoull(e, nullptr, 10));
	if (need + BS_MARGIN <= have) return true;
	counts[7] += 1;
	g_bs_refused_need = need + BS_MARGIN;
	return false;
}

// what the host path answers for a file whose header the leading blocks do not give: the first bad block (mi355x_bgzf_inflate over the
// whole file also reports what bgzf_in_plan found: a header that is none, a block that the file cuts off), else the header's code
int64_t header_code(const uint8_t *bam, size_t len, uint64_t u)
{
	std::vector<uint8_t> text((size_t)u + 1);
	const int64_t r = mi355x_bgzf_inflate(bam, len, (char *)text.data(), (size_t)u + 1);
	if (r < 0) return r;
	bsort::Header h;
	const int64_t hs = bsort::parse_header(text.data(), u, h);
	return hs < 0 ? hs : -(int64_t)u - 1;
}

// what the sort and the stand-alone index share: the file's plan, its header, the resident inflated stream and the count pass
struct Loaded {
	std::vector<int64_t> blk, txt;
	int64_t bad = -1;
	size_t n_blk = 0, need1 = 0;
	uint64_t u = 0;
	bsort::Header h;
	std::vector<uint8_t> lead;   // the leading blocks' bytes, as far as the header reaches
	double ms_inflate = 0;
};

// the plan and the header, from as many leading blocks as it takes (1, 2, 4, ...): on the host, before the lock.  false: *code is the call's
bool load_header(const char *who, const uint8_t *bam, size_t len, Loaded &L, int64_t *code)
{
	L.bad = bgzf_in_plan(bam, len, L.blk, L.txt);
	L.n_blk = L.blk.size() - 1;
	L.u = (uint64_t)L.txt[L.n_blk];
	if (L.n_blk >= (size_t)INT_MAX) die("%s: %zu blocks", who, L.n_blk);
	for (size_t k = 1;; k *= 2) {
		const size_t nb = std::min(k, L.n_blk);
		L.lead.resize((size_t)L.txt[nb] + 1);
		const int64_t r = nb ? mi355x_bgzf_inflate(bam, (size_t)L.blk[nb], (char *)L.lead.data(), L.lead.size()) : 0;
		if (r < 0) { *code = r; return false; }   // (the first bad block of the file: every block before it is among these)
		const int64_t hs = bsort::parse_header(L.lead.data(), (uint64_t)L.txt[nb], L.h);
		if (hs == 0) break;
		if (hs < 0 || nb == L.n_blk) { *code = header_code(bam, len, L.u); return false; }
	}
	return true;
}

// under the lock: the first admission check, the buffers, and every block inflated into d_u.  false: *code is the call's (INT64_MIN: refused)
bool load_inflate(SortCtx &C, const uint8_t *bam, Loaded &L, std::atomic<uint64_t> *counts, int64_t *code)
{
	const std::vector<int64_t> &blk = L.blk, &txt = L.txt;
	const size_t n_blk = L.n_blk;
	const uint64_t u = L.u;
	L.need1 = SortCtx::fixed_bytes() + (size_t)u + bsort::BAM_SORT_SLACK + (n_blk + 1) * (sizeof(uint64_t) + 3 * sizeof(uint32_t));
	if (!admitted(L.need1, counts)) { *code = INT64_MIN; return false; }
	if (!C.ready) C.init();
	C.d_u.ensure((size_t)u + bsort::BAM_SORT_SLACK);
	C.d_text_off.ensure((n_blk + 1) * sizeof(uint64_t));
	C.d_status.ensure((n_blk + 1) * sizeof(uint32_t));
	C.d_cnt.ensure((n_blk + 1) * sizeof(uint32_t));
	C.d_first.ensure((n_blk + 1) * sizeof(uint32_t));
	C.h_status.ensure((n_blk + 1) * sizeof(uint32_t));
	uint8_t *const d_u = (uint8_t *)C.d_u.p;

	auto t0 = std::chrono::steady_clock::now();
	HIP_OK(hipMemsetAsync(d_u + u, 0, bsort::BAM_SORT_SLACK, C.st[0]));
	const size_t n_groups = (n_blk + BS_GROUP - 1) / BS_GROUP;
	for (size_t g = 0; g < n_groups; ++g) {
		const int s = (int)(g & 1);
		const size_t b0 = g * BS_GROUP, b1 = std::min(n_blk, b0 + BS_GROUP);
		if (g >= 2) HIP_OK(hipEventSynchronize(C.ev[s]));   // the group before last on this stream has left the page-locked buffers
		C.in[s].queue(C.st[s], bam, blk.data(), txt.data(), b0, b1, d_u + txt[b0], (uint32_t *)C.d_status.p + b0, C.ev[s]);
	}
	HIP_OK(hipStreamSynchronize(C.st[1]));
	if (n_blk) HIP_OK(hipMemcpyAsync(C.h_status.p, C.d_status.p, n_blk * sizeof(uint32_t), hipMemcpyDeviceToHost, C.st[0]));
	HIP_OK(hipStreamSynchronize(C.st[0]));
	for (size_t b = 0; b < n_blk; ++b)
		if (((const uint32_t *)C.h_status.p)[b]) { *code = -blk[b] - 1; return false; }
	if (L.bad >= 0) { *code = -L.bad - 1; return false; }
	L.ms_inflate = ms_since(t0);
	return true;
}

// the count pass of the walk: the records, and whether the host has to walk (a foreign writer's blocks, or a malformed record)
void walk_count(SortCtx &C, const Loaded &L, bool *host_walk, size_t *n_rec)
{
	const size_t n_blk = L.n_blk;
	HIP_OK(hipMemcpyAsync(C.d_text_off.p, L.txt.data(), (n_blk + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, C.st[0]));
	HIP_OK(hipMemsetAsync(C.d_flag.p, 0, 16, C.st[0]));
	C.d_tmp.ensure(bam_sort_temp_bytes(0, (int)n_blk));
	launch_bam_sort_count(C.st[0], (const uint8_t *)C.d_u.p, (const uint64_t *)C.d_text_off.p, (int)n_blk, L.h.end, L.h.n_ref, (uint32_t *)C.d_cnt.p, (uint32_t *)C.d_flag.p);
	launch_bam_sort_scan(C.st[0], C.d_tmp.p, C.d_tmp.cap, (const uint32_t *)C.d_cnt.p, (uint32_t *)C.d_first.p, (int)n_blk);
	uint32_t *hf = (uint32_t *)C.h_flag.p;
	HIP_OK(hipMemcpyAsync(hf, C.d_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, C.st[0]));
	HIP_OK(hipMemcpyAsync(hf + 1, (const uint32_t *)C.d_first.p + n_blk, sizeof(uint32_t), hipMemcpyDeviceToHost, C.st[0]));
	HIP_OK(hipStreamSynchronize(C.st[0]));
	*host_walk = hf[0] != 0;
	*n_rec = hf[1];
}

// what the index stages need of device memory before the runs and the windows are counted
size_t index_need(size_t n_rec, int32_t n_ref, size_t n_cut)
{
	return IX_REC_BYTES * (n_rec + 1) + IX_REF_BYTES * ((size_t)n_ref + 1) + sizeof(uint64_t) * (n_cut + 1);
}

enum : int { IXB_OK = 0, IXB_FAILS = 1, IXB_REFUSED = 2, IXB_HOST = 3 };

// The index stages over the n_rec records of a stream on the device (BamIndexBufs, device.h): `cut` are the indexed file's blocks in its
// stream (d_cut: the same on the device, cut.size() words).  need: the call's device memory so far, index_need included.
// IXB_OK: P is filled (block-number space); IXB_FAILS: *bad_off is the smallest offset in d_u of a record that ends beyond 2^29 or,
// with keys, sorts before its predecessor; IXB_REFUSED: no memory for the runs and the windows; IXB_HOST: more windows than the device
// path counts (32-bit), the host indexes.
int index_build(SortCtx &C, const uint64_t *d_off, const uint32_t *d_order, const uint64_t *d_place, uint64_t place_base, const uint64_t *d_cut,
                const std::vector<uint64_t> &cut, size_t n_rec, int32_t n_ref, const uint64_t *d_keys, size_t need, std::atomic<uint64_t> *counts, bidx::Parts &P,
                uint64_t *bad_off, double *kernel_ms)
{
	if (std::min<uint64_t>(n_rec, (uint64_t)n_ref) >= ((uint64_t)1 << 17)) return IXB_HOST;   // (a contig has at most 2^15 windows)
	hipStream_t st = C.st[0];
	const size_t nr = n_rec + 1, nc = (size_t)n_ref + 1;
	C.x_rb.ensure(nr * 8); C.x_v0.ensure(nr * 8); C.x_mx.ensure(nr * 8); C.x_mxs.ensure(nr * 8);
	C.x_beg.ensure(nr * 4); C.x_map.ensure(nr * 4); C.x_maps.ensure(nr * 4); C.x_head.ensure(nr); C.x_rs.ensure(nr * 4); C.x_nsel.ensure(16);
	C.x_stat.ensure(nc * 32); C.x_nintv.ensure(nc * 4); C.x_woff.ensure(nc * 4);
	C.d_tmp.ensure(bam_index_temp_bytes((uint32_t)n_rec, n_ref, (uint32_t)n_rec));
	BamIndexBufs B = {};
	B.u = (const uint8_t *)C.d_u.p; B.off = d_off; B.order = d_order; B.place = d_place; B.place_base = place_base; B.cut = d_cut; B.n_cut = cut.size() - 1;
	B.n_rec = (uint32_t)n_rec; B.n_ref = n_ref; B.keys = d_keys; B.end_v = bidx::end_voffset(cut.data(), cut.size() - 1);
	B.rb = (uint64_t *)C.x_rb.p; B.v0 = (uint64_t *)C.x_v0.p; B.mx = (uint64_t *)C.x_mx.p; B.mxs = (uint64_t *)C.x_mxs.p;
	B.beg = (uint32_t *)C.x_beg.p; B.map = (uint32_t *)C.x_map.p; B.maps = (uint32_t *)C.x_maps.p; B.head = (uint8_t *)C.x_head.p;
	B.rs = (uint32_t *)C.x_rs.p; B.n_sel = (uint32_t *)C.x_nsel.p;
	B.stat = (uint64_t *)C.x_stat.p; B.n_intv = (uint32_t *)C.x_nintv.p; B.woff = (uint32_t *)C.x_woff.p;
	B.bad = (unsigned long long *)C.d_flag.p + 1; B.tmp = C.d_tmp.p; B.tmp_bytes = C.d_tmp.cap;
	HIP_OK(hipMemsetAsync(B.bad, 0xff, sizeof(unsigned long long), st));
	HIP_OK(hipEventRecord(C.ev_g[0][0], st));
	launch_bam_index_records(st, B);
	HIP_OK(hipEventRecord(C.ev_g[0][1], st));
	uint32_t n_runs = 0, n_win = 0;
	unsigned long long bad = 0;
	HIP_OK(hipMemcpyAsync(&n_runs, B.n_sel, sizeof n_runs, hipMemcpyDeviceToHost, st));
	HIP_OK(hipMemcpyAsync(&n_win, B.woff + n_ref, sizeof n_win, hipMemcpyDeviceToHost, st));
	HIP_OK(hipMemcpyAsync(&bad, B.bad, sizeof bad, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (bad != ~0ull) { *bad_off = bad; return IXB_FAILS; }
	if (!admitted(need + IX_RUN_BYTES * (size_t)n_runs + IX_WIN_BYTES * (size_t)n_win, counts)) return IXB_REFUSED;
	C.x_rk.ensure((size_t)n_runs * 8 + 8); C.x_rk2.ensure((size_t)n_runs * 8 + 8); C.x_ri.ensure((size_t)n_runs * 4 + 4); C.x_ri2.ensure((size_t)n_runs * 4 + 4);
	C.x_rbeg.ensure((size_t)n_runs * 8 + 8); C.x_rend.ensure((size_t)n_runs * 8 + 8); C.x_io.ensure((size_t)n_win * 8 + 8);
	B.rk = (uint64_t *)C.x_rk.p; B.rk2 = (uint64_t *)C.x_rk2.p; B.ri = (uint32_t *)C.x_ri.p; B.ri2 = (uint32_t *)C.x_ri2.p;
	B.rbeg = (uint64_t *)C.x_rbeg.p; B.rend = (uint64_t *)C.x_rend.p; B.io = (uint64_t *)C.x_io.p;
	HIP_OK(hipEventRecord(C.ev_g[1][0], st));
	launch_bam_index_runs(st, B, n_runs, n_win);
	HIP_OK(hipEventRecord(C.ev_g[1][1], st));
	P.n_ref = n_ref;
	P.run_key.resize(n_runs); P.run_beg.resize(n_runs); P.run_end.resize(n_runs);
	P.stat.resize(4 * nc); P.n_intv.resize(nc); P.ioffset.resize(n_win);
	if (n_runs) {
		HIP_OK(hipMemcpyAsync(P.run_key.data(), B.rk2, (size_t)n_runs * 8, hipMemcpyDeviceToHost, st));
		HIP_OK(hipMemcpyAsync(P.run_beg.data(), B.rbeg, (size_t)n_runs * 8, hipMemcpyDeviceToHost, st));
		HIP_OK(hipMemcpyAsync(P.run_end.data(), B.rend, (size_t)n_runs * 8, hipMemcpyDeviceToHost, st));
	}
	HIP_OK(hipMemcpyAsync(P.stat.data(), B.stat, nc * 32, hipMemcpyDeviceToHost, st));
	HIP_OK(hipMemcpyAsync(P.n_intv.data(), B.n_intv, nc * 4, hipMemcpyDeviceToHost, st));
	if (n_win) HIP_OK(hipMemcpyAsync(P.ioffset.data(), B.io, (size_t)n_win * 8, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	P.n_no_coor = P.stat[4 * (size_t)n_ref];
	P.stat.resize(4 * (size_t)n_ref); P.n_intv.resize((size_t)n_ref);
	float a = 0, b = 0;
	HIP_OK(hipEventElapsedTime(&a, C.ev_g[0][0], C.ev_g[0][1]));
	HIP_OK(hipEventElapsedTime(&b, C.ev_g[1][0], C.ev_g[1][1]));
	*kernel_ms = (double)a + (double)b;
	return IXB_OK;
}

// what a call that also indexes gets back
struct IndexWant {
	std::vector<uint8_t> bai;
	int reason = 0;
};

void index_counts(size_t n_rec, bool host_walk, const bidx::Parts &P, size_t n_runs, size_t bai_bytes)
{
	g_ix_counts[1] += n_rec; g_ix_counts[2] += host_walk ? 1 : 0; g_ix_counts[3] += n_runs; g_ix_counts[4] += P.n_chunks; g_ix_counts[5] += P.ioffset.size();
	g_ix_counts[6] += bai_bytes;
}

int64_t sort_dev(const uint8_t *bam, size_t len, uint8_t *out, size_t cap, IndexWant *ix)
{
	const auto t_all = std::chrono::steady_clock::now();
	std::atomic<uint64_t> *const refusals = g_bs_counts;
	Loaded L;
	int64_t code = 0;
	if (!load_header("mi355x_bam_sort_dev", bam, len, L, &code)) return code;
	const size_t n_blk = L.n_blk;
	const uint64_t u = L.u;
	const bsort::Header &h = L.h;
	std::vector<uint8_t> head;
	bsort::coordinate_header(L.lead.data(), h, head);
	const uint64_t hn = head.size();
	std::vector<uint8_t>().swap(L.lead);

	use_device();
	std::lock_guard<std::mutex> hold(g_bs_mu);
	SortCtx &C = g_bs;
	if (!load_inflate(C, bam, L, refusals, &code)) return code;
	const size_t need1 = L.need1;
	const double ms_inflate = L.ms_inflate;
	uint8_t *const d_u = (uint8_t *)C.d_u.p;

	// ---- walk ----
	auto t0 = std::chrono::steady_clock::now();
	bool host_walk = false;
	size_t n_rec = 0;
	walk_count(C, L, &host_walk, &n_rec);
	std::vector<uint64_t> h_off, h_key;
	std::vector<uint32_t> h_size;
	if (host_walk) {   // a foreign writer's blocks, or a malformed record: the host's hop decides which
		std::vector<uint8_t> text((size_t)u + 1);
		const int64_t r = mi355x_bgzf_inflate(bam, len, (char *)text.data(), (size_t)u + 1);
		if (r < 0) return r;
		const int64_t ws = bam_sort_walk(text.data(), h.end, u, h.n_ref, h_off, h_size, h_key);
		if (ws < 0) return ws;
		n_rec = h_off.size();
	}
	if ((uint64_t)cap < bam_sort_bound_of(u)) return 0;
	if (n_rec >= (size_t)INT_MAX - 1) {   // beyond the sort's 32-bit indices: refused like a file that does not fit
		g_bs_counts[7] += 1;
		g_bs_refused_need = need1 + BS_REC_BYTES * (n_rec + 1) + BS_MARGIN;
		return INT64_MIN;
	}
	size_t tmp_bytes = bam_sort_temp_bytes((uint32_t)n_rec, (int)n_blk);
	size_t need2 = need1 + BS_REC_BYTES * (n_rec + 1);
	if (ix) {   // the index stages' arrays, and the cuts of at most as many output blocks as the bound counts
		tmp_bytes = std::max(tmp_bytes, bam_index_temp_bytes((uint32_t)n_rec, h.n_ref, (uint32_t)n_rec));
		need2 += index_need(n_rec, h.n_ref, (size_t)(3 * ((u + bsort::BAM_SORT_HEADER_GROWTH) / 0xff00 + 1) + 3));
	}
	need2 += tmp_bytes;
	if (!admitted(need2)) return INT64_MIN;
	C.d_off.ensure((n_rec + 1) * sizeof(uint64_t));
	C.d_size.ensure((n_rec + 1) * sizeof(uint32_t));
	C.d_key.ensure((n_rec + 1) * sizeof(uint64_t));
	C.d_key2.ensure((n_rec + 1) * sizeof(uint64_t));
	C.d_idx.ensure((n_rec + 1) * sizeof(uint32_t));
	C.d_idx2.ensure((n_rec + 1) * sizeof(uint32_t));
	C.d_ssize.ensure((n_rec + 1) * sizeof(uint32_t));
	C.h_ssize.ensure((n_rec + 1) * sizeof(uint32_t));
	C.d_tmp.ensure(tmp_bytes);
	if (host_walk) {
		if (n_rec) {
			HIP_OK(hipMemcpyAsync(C.d_off.p, h_off.data(), n_rec * sizeof(uint64_t), hipMemcpyHostToDevice, C.st[0]));
			HIP_OK(hipMemcpyAsync(C.d_size.p, h_size.data(), n_rec * sizeof(uint32_t), hipMemcpyHostToDevice, C.st[0]));
			HIP_OK(hipMemcpyAsync(C.d_key.p, h_key.data(), n_rec * sizeof(uint64_t), hipMemcpyHostToDevice, C.st[0]));
		}
	} else
		launch_bam_sort_write(C.st[0], d_u, (const uint64_t *)C.d_text_off.p, (int)n_blk, h.end, h.n_ref, (const uint32_t *)C.d_first.p, (uint64_t *)C.d_off.p,
		                      (uint32_t *)C.d_size.p, (uint64_t *)C.d_key.p);
	HIP_OK(hipStreamSynchronize(C.st[0]));
	const double ms_walk = ms_since(t0);

	// ---- sort ----
	t0 = std::chrono::steady_clock::now();
	uint64_t *const d_dst = (uint64_t *)C.d_key.p;   // the keys' buffer again, once they are sorted
	launch_bam_sort_order(C.st[0], C.d_tmp.p, C.d_tmp.cap, (uint32_t)n_rec, (int)bsort::key_bits(h.n_ref), (const uint64_t *)C.d_key.p, (uint64_t *)C.d_key2.p,
	                      (uint32_t *)C.d_idx.p, (uint32_t *)C.d_idx2.p, (const uint32_t *)C.d_size.p, (uint32_t *)C.d_ssize.p, d_dst);
	HIP_OK(hipMemcpyAsync(C.h_ssize.p, C.d_ssize.p, (n_rec + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, C.st[0]));
	HIP_OK(hipStreamSynchronize(C.st[0]));
	const double ms_sort = ms_since(t0);

	// ---- emit ----
	t0 = std::chrono::steady_clock::now();
	std::vector<uint64_t> rec_off(n_rec + 1);
	rec_off[0] = 0;
	for (size_t i = 0; i < n_rec; ++i) rec_off[i + 1] = rec_off[i] + ((const uint32_t *)C.h_ssize.p)[i];
	if (rec_off[n_rec] != u - h.end) die("mi355x_bam_sort_dev: the sorted records have %llu bytes, the stream %llu", (unsigned long long)rec_off[n_rec], (unsigned long long)(u - h.end));
	std::vector<size_t> cut;
	bam_sort_cuts(hn, rec_off, cut);
	const size_t n_out = cut.size() - 1, n_pieces = (n_out + BAM_DEV_BLOCKS - 1) / BAM_DEV_BLOCKS;
	// ---- index (mi355x_bam_sort_index_dev only): from the order and the cuts, before anything is written to out ----
	bidx::Parts parts;
	double ms_index = 0, ix_kernel_ms = 0;
	bool ix_host = false;
	std::vector<int64_t> out_off;   // the output blocks' file offsets
	if (ix) {
		const auto ti = std::chrono::steady_clock::now();
		const std::vector<uint64_t> cut64(cut.begin(), cut.end());
		C.x_cut.ensure(cut64.size() * sizeof(uint64_t));
		C.lane[0].want_sizes(); C.lane[1].want_sizes();
		HIP_OK(hipMemcpyAsync(C.x_cut.p, cut64.data(), cut64.size() * sizeof(uint64_t), hipMemcpyHostToDevice, C.st[0]));
		uint64_t bad_off = 0;
		const int r = index_build(C, (const uint64_t *)C.d_off.p, (const uint32_t *)C.d_idx2.p, d_dst, hn, (const uint64_t *)C.x_cut.p, cut64, n_rec, h.n_ref, nullptr,
		                          need2, refusals, parts, &bad_off, &ix_kernel_ms);
		if (r == IXB_FAILS) { ix->reason = bidx::BAI_TOO_LONG; return -(int64_t)bad_off - 1; }
		if (r == IXB_REFUSED) return INT64_MIN;
		ix_host = r == IXB_HOST;
		out_off.reserve(n_out + 1);
		ms_index = ms_since(ti);
	}
	double gather_ms = 0;
	uint64_t gather_bytes = 0, piece_gather[2] = {0, 0};
	const bool gather_alone = getenv("MPIBWA_BAM_SORT_GATHER_ALONE") != nullptr;   // tools/bench_bam_sort.py: no other kernel beside a timed gather
	auto start = [&](size_t k) {   // everything of a piece, queued on the piece's stream
		const int s = (int)(k & 1);
		const size_t b0 = k * BAM_DEV_BLOCKS, b1 = std::min(n_out, b0 + BAM_DEV_BLOCKS);
		const uint64_t p0 = cut[b0], p1 = cut[b1];   // (p1 - p0 <= BAM_DEV_BYTES: a block has at most 0xff00 bytes)
		uint8_t *const d_piece = (uint8_t *)C.d_piece[s].p;
		if (p0 < hn)   // (pageable memory: the copy is staged by the runtime and has left head when the call returns)
			HIP_OK(hipMemcpyAsync(d_piece, head.data() + p0, (size_t)(std::min(p1, hn) - p0), hipMemcpyHostToDevice, C.st[s]));
		piece_gather[s] = 0;
		if (p1 > hn) {
			const uint64_t lo = std::max(p0, hn) - hn, hi = p1 - hn;   // of the sorted records
			const size_t r0 = (size_t)(std::upper_bound(rec_off.begin(), rec_off.end(), lo) - rec_off.begin()) - 1;
			const size_t r1 = (size_t)(std::lower_bound(rec_off.begin(), rec_off.end(), hi) - rec_off.begin());
			if (gather_alone) HIP_OK(hipStreamSynchronize(C.st[s ^ 1]));
			HIP_OK(hipEventRecord(C.ev_g[s][0], C.st[s]));
			launch_bam_sort_gather(C.st[s], d_u, (const uint64_t *)C.d_off.p, (const uint32_t *)C.d_idx2.p, d_dst, (uint32_t)n_rec, (uint32_t)r0, (uint32_t)r1, lo, hi,
			                       d_piece + (std::max(p0, hn) - p0));
			HIP_OK(hipEventRecord(C.ev_g[s][1], C.st[s]));
			piece_gather[s] = hi - lo;
		}
		C.lane[s].cuts_up(C.st[s], cut.data() + b0, (int)(b1 - b0));
		C.lane[s].queue(C.st[s], d_piece, (int)(b1 - b0));
	};
	size_t w = 0;
	if (n_pieces) start(0);
	for (size_t k = 0; k < n_pieces; ++k) {
		const int s = (int)(k & 1);
		if (k + 1 < n_pieces) start(k + 1);   // (the other stream: its kernels run beside this piece's way back)
		HIP_OK(hipStreamSynchronize(C.st[s]));
		if (piece_gather[s]) {
			float ms = 0;
			HIP_OK(hipEventElapsedTime(&ms, C.ev_g[s][0], C.ev_g[s][1]));
			gather_ms += ms; gather_bytes += piece_gather[s];
		}
		DeflateLane &Z = C.lane[s];
		const size_t zbytes = Z.packed();
		if (w + zbytes + 28 > cap) die("mi355x_bam_sort_dev: %zu bytes of blocks above the bound %zu", w + zbytes + 28, (size_t)bam_sort_bound_of(u));
		const size_t nb_k = std::min(n_out, (k + 1) * BAM_DEV_BLOCKS) - k * BAM_DEV_BLOCKS;
		Z.fetch(C.st[s], ix ? nb_k : 0);
		HIP_OK(hipStreamSynchronize(C.st[s]));
		if (ix) {   // the piece's blocks, one by one
			size_t at = w;
			for (size_t j = 0; j < nb_k; ++j) { out_off.push_back((int64_t)at); at += ((const uint32_t *)Z.h_sizes.p)[j]; }
			if (at != w + zbytes) die("mi355x_bam_sort_index_dev: a piece's blocks have %zu bytes, the piece %zu", at - w, zbytes);
		}
		w += Z.store(out + w);
	}
	if (ix) out_off.push_back((int64_t)w);
	w += mi355x_bgzf_eof(out + w);
	const double ms_emit = ms_since(t0) - ms_index;
	if (ix) {
		const auto ts = std::chrono::steady_clock::now();
		size_t n_runs = parts.run_key.size();
		if (ix_host) {   // more windows than the device path counts: the host indexes what was written
			const int64_t r = bam_index_host(out, w, ix->bai, &ix->reason);
			if (r != (int64_t)n_rec) die("mi355x_bam_sort_index_dev: the host indexed %lld records of %zu", (long long)r, n_rec);
			n_runs = 0;
		} else
			bidx::serialise(parts, out_off.data(), ix->bai);
		g_ix_counts[2] += ix_host ? 1 : 0;
		index_counts(n_rec, false, parts, n_runs, ix->bai.size());
		std::lock_guard<std::mutex> lk(g_ix_ms_mu);
		const double v[8] = {ms_inflate, ms_walk, ms_index, ms_since(ts), ms_since(t_all), ix_kernel_ms, 0, 0};
		memcpy(g_ix_ms, v, sizeof v);
	}

	g_bs_counts[1] += n_rec; g_bs_counts[2] += host_walk ? 1 : 0; g_bs_counts[3] += u; g_bs_counts[4] += n_blk; g_bs_counts[5] += n_out + 1; g_bs_counts[6] += w;
	{
		std::lock_guard<std::mutex> lk(g_bs_ms_mu);
		const double v[8] = {ms_inflate, ms_walk, ms_sort, ms_emit, ms_since(t_all), gather_ms, (double)gather_bytes, 0};
		memcpy(g_bs_ms, v, sizeof v);
	}
	return (int64_t)w;
}

// 1 for a negative code of the sort that a BGZF block caused, 2 for one that the header or a record caused (a failing file is inflated
// once more on the host to tell)
int sort_failure_reason(const uint8_t *bam, size_t len)
{
	std::vector<int64_t> blk, txt;
	const int64_t bad = bgzf_in_plan(bam, len, blk, txt);
	std::vector<uint8_t> text((size_t)txt.back() + 1);
	const int64_t r = mi355x_bgzf_inflate(bam, len, (char *)text.data(), text.size());
	return r < 0 || bad >= 0 ? bidx::BAI_BAD_BLOCK : bidx::BAI_BAD_RECORD;
}

// mi355x_bam_index_dev: the inflate and the walk of the sort, then the index stages with the file's own order and blocks.  Whatever
// fails or does not suit the device goes to the host path, which decides the code.
int64_t index_dev(const uint8_t *bam, size_t len, std::vector<uint8_t> &bai, int *reason)
{
	const auto t_all = std::chrono::steady_clock::now();
	Loaded L;
	int64_t code = 0;
	auto by_host = [&]() {
		g_ix_counts[2] += 1;
		const int64_t n = bam_index_host(bam, len, bai, reason);
		if (n >= 0) { g_ix_counts[1] += (uint64_t)n; g_ix_counts[6] += bai.size(); }
		return n;
	};
	if (!load_header("mi355x_bam_index_dev", bam, len, L, &code)) return bam_index_host(bam, len, bai, reason);
	std::vector<uint8_t>().swap(L.lead);
	use_device();
	std::unique_lock<std::mutex> hold(g_bs_mu);
	SortCtx &C = g_bs;
	if (!load_inflate(C, bam, L, g_ix_counts, &code)) {
		hold.unlock();
		return code == INT64_MIN ? code : bam_index_host(bam, len, bai, reason);
	}
	auto t0 = std::chrono::steady_clock::now();
	bool host_walk = false;
	size_t n_rec = 0;
	walk_count(C, L, &host_walk, &n_rec);
	if (host_walk) {   // a foreign writer's blocks, or a malformed record
		hold.unlock();
		return by_host();
	}
	if (n_rec >= (size_t)INT_MAX - 1) {
		g_ix_counts[7] += 1;
		return INT64_MIN;
	}
	const size_t n_blk = L.n_blk;
	const size_t tmp_bytes = std::max(bam_sort_temp_bytes((uint32_t)n_rec, (int)n_blk), bam_index_temp_bytes((uint32_t)n_rec, L.h.n_ref, (uint32_t)n_rec));
	const size_t need2 = L.need1 + (sizeof(uint64_t) + sizeof(uint32_t) + sizeof(uint64_t)) * (n_rec + 1) + index_need(n_rec, L.h.n_ref, 0) + tmp_bytes;
	if (!admitted(need2, g_ix_counts)) return INT64_MIN;
	C.d_off.ensure((n_rec + 1) * sizeof(uint64_t));
	C.d_size.ensure((n_rec + 1) * sizeof(uint32_t));
	C.d_key.ensure((n_rec + 1) * sizeof(uint64_t));
	C.d_tmp.ensure(tmp_bytes);
	launch_bam_sort_write(C.st[0], (const uint8_t *)C.d_u.p, (const uint64_t *)C.d_text_off.p, (int)n_blk, L.h.end, L.h.n_ref, (const uint32_t *)C.d_first.p,
	                      (uint64_t *)C.d_off.p, (uint32_t *)C.d_size.p, (uint64_t *)C.d_key.p);
	HIP_OK(hipStreamSynchronize(C.st[0]));
	const double ms_walk = ms_since(t0);

	t0 = std::chrono::steady_clock::now();
	const std::vector<uint64_t> cut(L.txt.begin(), L.txt.end());
	bidx::Parts parts;
	uint64_t bad_off = 0;
	double kernel_ms = 0;
	const int r = index_build(C, (const uint64_t *)C.d_off.p, nullptr, (const uint64_t *)C.d_off.p, 0, (const uint64_t *)C.d_text_off.p, cut, n_rec, L.h.n_ref,
	                          (const uint64_t *)C.d_key.p, need2, g_ix_counts, parts, &bad_off, &kernel_ms);
	if (r == IXB_REFUSED) return INT64_MIN;
	if (r != IXB_OK) {   // out of order, beyond 2^29, or more windows than the device counts
		hold.unlock();
		return by_host();
	}
	const double ms_index = ms_since(t0);
	hold.unlock();
	t0 = std::chrono::steady_clock::now();
	const size_t n_runs = parts.run_key.size();
	bidx::serialise(parts, L.blk.data(), bai);
	index_counts(n_rec, false, parts, n_runs, bai.size());
	*reason = bidx::BAI_OK;
	std::lock_guard<std::mutex> lk(g_ix_ms_mu);
	const double v[8] = {L.ms_inflate, ms_walk, ms_index, ms_since(t0), ms_since(t_all), kernel_ms, 0, 0};
	memcpy(g_ix_ms, v, sizeof v);
	return (int64_t)n_rec;
}

} // namespace

void release_bam_sort_contexts()
{
	if (!g_bs_mu.try_lock()) return;   // a sort is running: its buffers stay
	if (g_bs.ready) g_bs.release();
	g_bs_mu.unlock();
}

} // namespace mbw

using namespace mbw;

// mi355x_bam_sort on the device: the same record stream, cuts and return codes; the device deflate's one setting (include/mpibwa_amd.h)
extern "C" int64_t mi355x_bam_sort_dev(const uint8_t *bam, size_t len, uint8_t *out, size_t cap)
{
	g_bs_counts[0] += 1;
	return sort_dev(bam, len, out, cap, nullptr);
}

// the sort and, from what it holds on the device, the BAI index of what it writes (include/mpibwa_amd.h)
extern "C" int64_t mi355x_bam_sort_index_dev(const uint8_t *bam, size_t len, uint8_t *out, size_t cap, uint8_t **bai, size_t *bai_len, int *reason)
{
	g_bs_counts[0] += 1; g_ix_counts[0] += 1;
	IndexWant ix;
	const int64_t n = sort_dev(bam, len, out, cap, &ix);
	if (reason) *reason = n >= 0 || n == INT64_MIN ? bidx::BAI_OK : ix.reason ? ix.reason : sort_failure_reason(bam, len);
	if (n == INT64_MIN) g_ix_counts[7] += 1;
	if (n > 0) bam_index_hand_over(ix.bai, bai, bai_len);
	return n;
}

extern "C" int64_t mi355x_bam_index_dev(const uint8_t *bam, size_t len, uint8_t **bai, size_t *bai_len, int *reason)
{
	g_ix_counts[0] += 1;
	std::vector<uint8_t> bytes;
	int why = 0;
	const int64_t n = index_dev(bam, len, bytes, &why);
	if (reason) *reason = n == INT64_MIN ? 0 : why;
	if (n >= 0) bam_index_hand_over(bytes, bai, bai_len);
	return n;
}

extern "C" void mi355x_bam_index_dev_counts(uint64_t out[8])
{
	for (int k = 0; k < 8; ++k) out[k] = g_ix_counts[k].load();
}

// the last finished indexing call's stages, for tools/bench_bam_index.py: wall ms of inflate, walk, the index stages, the serialisation
// and the whole call; the index kernels' summed event ms; 0; 0
extern "C" void mi355x_bam_index_dev_stage_ms(double out[8])
{
	std::lock_guard<std::mutex> lk(g_ix_ms_mu);
	memcpy(out, g_ix_ms, sizeof g_ix_ms);
}

extern "C" void mi355x_bam_sort_dev_counts(uint64_t out[8])
{
	for (int k = 0; k < 8; ++k) out[k] = g_bs_counts[k].load();
}

// the last finished call's stages, for tools/bench_bam_sort.py: wall ms of inflate, walk, sort, emit and the whole call; the record gather
// kernels' summed event ms and the bytes they moved; 0
extern "C" void mi355x_bam_sort_dev_stage_ms(double out[8])
{
	std::lock_guard<std::mutex> lk(g_bs_ms_mu);
	memcpy(out, g_bs_ms, sizeof g_bs_ms);
}

// the bytes of device memory, margin included, that the last call refused for memory needed (0: none was refused)
extern "C" uint64_t mi355x_bam_sort_dev_refused_need(void)
{
	return g_bs_refused_need.load();
}
