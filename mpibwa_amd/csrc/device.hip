// device.hip — device management, index residency in HBM and the stage-level C entry points.
#include <hip/hip_runtime.h>
#include <atomic>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "device.h"
#include "host.h"
#include <cmath>

namespace mbw {

#define HIP_OK(call)                                                                                             \
	do {                                                                                                         \
		hipError_t e_ = (call);                                                                                  \
		if (e_ != hipSuccess) die("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);    \
	} while (0)

static DevIndex g_idx;
DevIndex &dev_index() { return g_idx; }
static std::atomic<unsigned long long> g_buf_growths(0);
void note_buffer_growth(size_t from, size_t to, const char *kind)
{
	++g_buf_growths;
	static const bool log = getenv("MPIBWA_GROWTH_LOG") != nullptr;
	if (log) fprintf(stderr, "[growth] %s buffer %zu -> %zu bytes (reallocation %llu)\n", kind, from, to, g_buf_growths.load());
}
// (re)allocations of device and page-locked work buffers so far: hipFree / hipMalloc / hipHostMalloc stall every stream of the
// device, so a caller that sees this number move in steady state knows where a slow chunk came from
extern "C" unsigned long long mi355x_buffer_growths(void) { return g_buf_growths.load(); }
std::vector<DevBuf *> *g_devbuf_owner = nullptr;
void *DevBuf::ensure(size_t bytes)
{
	if (bytes > cap) {
		size_t want = bytes + bytes / 4 + 256;
		note_buffer_growth(cap, want, "device");
		if (p) HIP_OK(hipFree(p));
		p = nullptr; cap = 0;
		// (what the runtime itself needs later — kernel scratch, queues, events — comes out of the same HBM, and it aborts the process
		// when it finds none: an allocation that leaves less than a reserve free counts as one that did not fit)
		static const size_t reserve = (size_t)(getenv("MPIBWA_HBM_RESERVE_GB") ? atof(getenv("MPIBWA_HBM_RESERVE_GB")) : 6.0) << 30;
		for (int attempt = 0;; ++attempt) {
			if (hipMalloc(&p, want) == hipSuccess) {
				size_t fr = 0, tot = 0;
				if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr >= reserve) break;
				(void)hipFree(p);
			}
			(void)hipGetLastError();
			p = nullptr;
			if (attempt == 0 && want > bytes + 256) { want = bytes + 256; continue; }   // without the head room first
			if (device_memory_pressure(want)) continue;
			size_t fr = 0, tot = 0;
			(void)hipMemGetInfo(&fr, &tot);
			die("device work buffer of %.2f GB does not fit: %.1f of %.1f GB free (index, dense SA and the work buffers of this call share the HBM; no other "
			    "call is in flight and no idle buffer is left to give back)", want / 1e9, fr / 1e9, tot / 1e9);
		}
		cap = want;
	}
	return p;
}
void DevBuf::release()
{
	if (p) (void)hipFree(p);
	p = nullptr; cap = 0;
}
void *PinBuf::ensure(size_t bytes)
{
	if (bytes > cap) {
		note_buffer_growth(cap, bytes + bytes / 4 + 4096, "page-locked");
		if (p) HIP_OK(hipHostFree(p));
		cap = bytes + bytes / 4 + 4096;
		HIP_OK(hipHostMalloc(&p, cap, hipHostMallocDefault));
	}
	return p;
}

static void require_device(int local_rank)
{
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n == 0)
		die("no HIP device visible: the alignment hot path runs on MI355X only, there is no CPU fallback");
	HIP_OK(hipSetDevice(local_rank % n));
	hipDeviceProp_t prop;
	HIP_OK(hipGetDeviceProperties(&prop, local_rank % n));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		die("device %d is %s; this library carries gfx950 (MI355X) code objects only", local_rank % n, prop.gcnArchName);
	g_idx.device = local_rank % n;
}

static uint64_t index_hash(const bwt_t *bwt, const bntseq_t *bns)
{
	uint64_t h = 1469598103934665603ull;   // FNV-1a
	auto mix = [&](const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
	for (int i = 0; i < bns->n_seqs; ++i) {
		mix(&bns->anns[i].offset, sizeof bns->anns[i].offset);
		mix(&bns->anns[i].len, sizeof bns->anns[i].len);
		if (bns->anns[i].name) mix(bns->anns[i].name, strlen(bns->anns[i].name));
	}
	if (bwt->bwt && bwt->bwt_size >= 16) mix(bwt->bwt, 64);
	return h;
}

// (called under index_mutex() on every mem_process_seqs call: the contig table — 10^5..10^6 names on some references — is only
// hashed again when the caller passes other pointers than the ones that matched last time)
static const void *g_last_ok[4] = {nullptr, nullptr, nullptr, nullptr};
static int g_last_ok_nseqs = -1;
bool index_matches(const bwt_t *bwt, const bntseq_t *bns, const char **what)
{
	const char *w = nullptr;
	const bool same_ptrs = g_last_ok[0] == bwt && g_last_ok[1] == bns && g_last_ok[2] == bns->anns && g_last_ok[3] == bwt->bwt && g_last_ok_nseqs == bns->n_seqs;
	if (bwt->seq_len != g_idx.id_seq_len) w = "seq_len";
	else if (bwt->primary != g_idx.id_primary) w = "primary";
	else if (memcmp(bwt->L2, g_idx.id_L2, sizeof g_idx.id_L2) != 0) w = "L2";
	else if (bns->l_pac != g_idx.l_pac) w = "l_pac";
	else if (bns->n_seqs != g_idx.id_n_seqs) w = "n_seqs";
	else if (!same_ptrs && index_hash(bwt, bns) != g_idx.id_hash) w = "contig table or BWT";
	if (!w) { g_last_ok[0] = bwt; g_last_ok[1] = bns; g_last_ok[2] = bns->anns; g_last_ok[3] = bwt->bwt; g_last_ok_nseqs = bns->n_seqs; }
	else g_last_ok[0] = nullptr;
	if (what) *what = w;
	return w == nullptr;
}

static void no_calls_in_flight(const char *who)
{
	if (calls_in_flight() > 0) die("%s while mem_process_seqs calls are in flight on the resident index", who);
}

static void alloc_index(const bwt_t *bwt, const bntseq_t *bns)
{
	std::lock_guard<std::recursive_mutex> lk(index_mutex());   // no call can pass its residency check while the buffers are replaced
	no_calls_in_flight("index upload");
	g_idx.ready = false;
	if (g_idx.d_blk) { (void)hipFree(g_idx.d_blk); (void)hipFree(g_idx.d_sa); (void)hipFree(g_idx.d_pac); }
	g_idx.blk_bytes = ((size_t)bwt->bwt_size * 4 + 63) / 64 * 64 + 64;   // whole 64-B blocks + one pad block
	g_idx.sa_bytes = (size_t)bwt->n_sa * 8;
	g_idx.pac_bytes = (size_t)bns->l_pac / 4 + 1 + 16;
	HIP_OK(hipMalloc(&g_idx.d_blk, g_idx.blk_bytes));
	HIP_OK(hipMalloc(&g_idx.d_sa, g_idx.sa_bytes));
	HIP_OK(hipMalloc(&g_idx.d_pac, g_idx.pac_bytes));
	HIP_OK(hipMemset(g_idx.d_blk, 0, g_idx.blk_bytes));
	HIP_OK(hipMemset(g_idx.d_pac, 0, g_idx.pac_bytes));
	FmDev &fm = g_idx.fm;
	fm.blk = g_idx.d_blk; fm.sa = (const uint64_t *)g_idx.d_sa; fm.sa_full = nullptr;
	fm.p3tab = nullptr; fm.p3_k = 0; fm.occ32 = nullptr; fm.occ_sb = nullptr; fm.kmt = nullptr; fm.kmt_k = 0;
	if (g_idx.d_occ32) { (void)hipFree(g_idx.d_occ32); g_idx.d_occ32 = nullptr; }
	if (g_idx.d_kmt) { (void)hipFree(g_idx.d_kmt); g_idx.d_kmt = nullptr; g_idx.kmt_bytes = 0; }
	if (g_idx.d_p3tab) { (void)hipFree(g_idx.d_p3tab); g_idx.d_p3tab = nullptr; }
	if (g_idx.d_sa_full) { (void)hipFree(g_idx.d_sa_full); g_idx.d_sa_full = nullptr; g_idx.sa_full_bytes = 0; }
	fm.primary = bwt->primary; fm.seq_len = bwt->seq_len;
	for (int i = 0; i < 5; ++i) fm.L2[i] = bwt->L2[i];
	int sh = 0;
	while ((1 << sh) < bwt->sa_intv) ++sh;
	if ((1 << sh) != bwt->sa_intv) die("SA sampling interval %d is not a power of two", bwt->sa_intv);
	fm.sa_shift = sh;
	g_idx.l_pac = bns->l_pac;
	g_idx.id_primary = bwt->primary; g_idx.id_seq_len = bwt->seq_len; g_idx.id_n_seqs = bns->n_seqs;
	g_idx.id_hash = index_hash(bwt, bns);
	g_last_ok[0] = nullptr;   // a new resident index: the next call hashes its contig table again
	memcpy(g_idx.id_L2, bwt->L2, sizeof g_idx.id_L2);
	if (bwt->seq_len >= (1ull << 34))
		die("reference of %llu symbols: this build packs SA-interval bounds into 34 bits (references up to 8.5 Gbp)", (unsigned long long)bwt->seq_len);
	// the buffers are handed to collectives on other streams next (RCCL, torch): the memsets above must have landed
	HIP_OK(hipDeviceSynchronize());
}

} // namespace mbw

using namespace mbw;

// Expand the sampled SA into a dense one when HBM allows it (MPIBWA_SA_DENSE=0 disables it).
// Jump table of the third seeding pass (fm_kernels.hip): 4^13 entries x 32 B = 2.1 GB, built in a few tens of ms.
// MPIBWA_P3TAB=0 disables it, MPIBWA_P3TAB=<k> chooses the number of extensions folded into it (default 12).
static void maybe_build_p3()
{
	int k = 12;
	if (const char *e = getenv("MPIBWA_P3TAB")) k = atoi(e);
	if (g_idx.d_p3tab) { (void)hipFree(g_idx.d_p3tab); g_idx.d_p3tab = nullptr; g_idx.fm.p3tab = nullptr; }
	if (k < 4 || k > 14) return;
	const size_t bytes = ((size_t)1 << (2 * (k + 1))) * 32;
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + ((size_t)16 << 30)) return;
	HIP_OK(hipMalloc(&g_idx.d_p3tab, bytes));
	launch_p3_build(0, g_idx.fm, k, g_idx.d_p3tab);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	g_idx.fm.p3tab = g_idx.d_p3tab;
	g_idx.fm.p3_k = k;
}

// The seeding kernel's k-mer tables (fm_kernels.hip: kmt_build_kernel): the bi-interval of every string of up to K bases, K chosen
// so that the longest table has about as many entries as the index has rows (beyond that a table entry is as cold as an occ block)
// and at most 14 (5.7 GB).  MPIBWA_KMT=<K> chooses K (0 = no tables: every extension through the occ table).
static void maybe_build_kmt()
{
	if (g_idx.d_kmt) { (void)hipFree(g_idx.d_kmt); g_idx.d_kmt = nullptr; g_idx.kmt_bytes = 0; }
	g_idx.fm.kmt = nullptr; g_idx.fm.kmt_k = 0;
	int k = 1;
	while (k < 14 && ((uint64_t)1 << (2 * k)) < g_idx.fm.seq_len) ++k;
	if (const char *e = getenv("MPIBWA_KMT")) k = atoi(e);
	if (k < 1) return;
	if (k > 15) k = 15;
	const size_t bytes = kmt_bytes(k);
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + ((size_t)16 << 30)) return;
	HIP_OK(hipMalloc(&g_idx.d_kmt, bytes));
	launch_kmt_build(0, g_idx.fm, k, g_idx.d_kmt);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	g_idx.kmt_bytes = bytes;
	g_idx.fm.kmt = g_idx.d_kmt;
	g_idx.fm.kmt_k = k;
}

// The seeding kernel's own occ table (fm_kernels.hip: occ32_build_kernel), derived on the device from the bwa-format blocks.
static void build_occ32()
{
	if (g_idx.d_occ32) { (void)hipFree(g_idx.d_occ32); g_idx.d_occ32 = nullptr; }
	g_idx.occ32_bytes = occ32_bytes(g_idx.fm.seq_len);
	HIP_OK(hipMalloc(&g_idx.d_occ32, g_idx.occ32_bytes));
	launch_occ32_build(0, g_idx.fm, g_idx.d_occ32);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
}

static void maybe_expand_sa()
{
	const char *e = getenv("MPIBWA_SA_DENSE");
	if (e && atoi(e) == 0) return;
	size_t need = (size_t)(g_idx.fm.seq_len + 1) * 8, free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + (need >> 1) + ((size_t)8 << 30)) return;   // keep room for the batches
	HIP_OK(hipMalloc(&g_idx.d_sa_full, need));
	unsigned long long *d_cnt;
	HIP_OK(hipMalloc(&d_cnt, 64));
	HIP_OK(hipMemset(d_cnt, 0, 64));
	hipEvent_t a, b;
	HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b));
	HIP_OK(hipEventRecord(a, 0));
	launch_sa_expand(0, g_idx.fm, (uint64_t *)g_idx.d_sa_full, d_cnt);
	HIP_OK(hipEventRecord(b, 0));
	HIP_OK(hipEventSynchronize(b));
	HIP_OK(hipGetLastError());
	float ms = 0;
	HIP_OK(hipEventElapsedTime(&ms, a, b));
	g_idx.sa_expand_ms = ms;
	g_idx.sa_full_bytes = need;
	g_idx.fm.sa_full = (const uint64_t *)g_idx.d_sa_full;
	(void)hipFree(d_cnt); (void)hipEventDestroy(a); (void)hipEventDestroy(b);
}

// GPUs this process can see (0 when there is none: callers decide how many ranks share a device)
extern "C" int mi355x_device_count(void)
{
	int n = 0;
	return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// free / total bytes of the device the index lives on (0 on success), through this library's own HIP runtime
extern "C" int mi355x_device_memory(size_t *free_bytes, size_t *total_bytes)
{
	size_t fr = 0, tot = 0;
	if (g_idx.device >= 0 && hipSetDevice(g_idx.device) != hipSuccess) return -1;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) return -1;
	if (free_bytes) *free_bytes = fr;
	if (total_bytes) *total_bytes = tot;
	return 0;
}

extern "C" int mi355x_index_alloc(int local_rank, const bwt_t *bwt, const bntseq_t *bns)
{
	require_device(local_rank);
	alloc_index(bwt, bns);   // buffers only: fill them with mi355x_index_d2d / ncclBroadcast, then mi355x_index_commit()
	return 0;
}

extern "C" int mi355x_index_upload(int local_rank, const bwt_t *bwt, const bntseq_t *bns, const uint8_t *pac)
{
	require_device(local_rank);
	alloc_index(bwt, bns);
	HIP_OK(hipMemcpy(g_idx.d_blk, bwt->bwt, (size_t)bwt->bwt_size * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(g_idx.d_sa, bwt->sa, g_idx.sa_bytes, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(g_idx.d_pac, pac, (size_t)bns->l_pac / 4 + 1, hipMemcpyHostToDevice));
	const bool dbg = getenv("MPIBWA_DEBUG") != nullptr;
	if (dbg) fprintf(stderr, "[upload] copied\n");
	build_occ32();
	if (dbg) fprintf(stderr, "[upload] occ32 built\n");
	maybe_expand_sa();
	if (dbg) fprintf(stderr, "[upload] SA expanded\n");
	maybe_build_p3();
	maybe_build_kmt();
	if (dbg) fprintf(stderr, "[upload] jump table and k-mer tables built\n");
	g_idx.ready = true;
	return 0;
}

extern "C" int mi355x_sa_batch(int n, const uint64_t *k, uint64_t *sa_out, double *kernel_ms, uint64_t *algo_bytes);
extern "C" int mi355x_index_buffers(void **d_bwt, size_t *bwt_bytes, void **d_sa, size_t *sa_bytes, void **d_pac,
                                    size_t *pac_bytes)
{
	if (!g_idx.d_blk) return -1;
	*d_bwt = g_idx.d_blk; *bwt_bytes = g_idx.blk_bytes;
	*d_sa = g_idx.d_sa; *sa_bytes = g_idx.sa_bytes;
	*d_pac = g_idx.d_pac; *pac_bytes = g_idx.pac_bytes;
	return 0;
}

// Copy `bytes` from a device pointer owned by the caller (e.g. a torch tensor that has just received an RCCL broadcast)
// into index buffer `which` (0 = occ blocks, 1 = sampled SA, 2 = pac), or out of it when to_index == 0.
extern "C" int mi355x_index_d2d(int which, void *ext, size_t bytes, int to_index)
{
	if (!g_idx.d_blk) return -1;
	void *buf = which == 0 ? g_idx.d_blk : which == 1 ? g_idx.d_sa : g_idx.d_pac;
	size_t cap = which == 0 ? g_idx.blk_bytes : which == 1 ? g_idx.sa_bytes : g_idx.pac_bytes;
	if (bytes > cap) return -2;
	HIP_OK(hipMemcpy(to_index ? buf : ext, to_index ? ext : buf, bytes, hipMemcpyDeviceToDevice));
	return 0;
}
// after the three buffers have been filled by broadcast: expand the dense SA and mark the index usable
extern "C" int mi355x_index_commit(void)
{
	if (!g_idx.d_blk) return -1;
	build_occ32();
	maybe_expand_sa();
	maybe_build_p3();
	maybe_build_kmt();
	g_idx.ready = true;
	return 0;
}

extern "C" void mi355x_finalize(void)
{
	std::lock_guard<std::recursive_mutex> lk(index_mutex());
	no_calls_in_flight("mi355x_finalize");
	if (g_idx.d_blk) { (void)hipFree(g_idx.d_blk); (void)hipFree(g_idx.d_sa); (void)hipFree(g_idx.d_pac); }
	if (g_idx.d_sa_full) (void)hipFree(g_idx.d_sa_full);
	if (g_idx.d_p3tab) (void)hipFree(g_idx.d_p3tab);
	if (g_idx.d_occ32) (void)hipFree(g_idx.d_occ32);
	if (g_idx.d_kmt) (void)hipFree(g_idx.d_kmt);
	g_idx = DevIndex();
	release_idle_work_buffers();   // a process that is done with this index gives the HBM of its call contexts back too
}

namespace mbw {

static void need_index()
{
	if (!g_idx.ready) die("index not resident on the device: call mi355x_index_upload() first");
}

struct Timer {
	hipEvent_t a, b;
	Timer() { HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); }
	~Timer() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
	void start(hipStream_t s) { HIP_OK(hipEventRecord(a, s)); }
	double stop(hipStream_t s)
	{
		HIP_OK(hipEventRecord(b, s));
		HIP_OK(hipEventSynchronize(b));
		float ms = 0;
		HIP_OK(hipEventElapsedTime(&ms, a, b));
		return ms;
	}
};

SmemParams smem_params(const mem_opt_t *opt)
{
	SmemParams sp;
	sp.min_seed_len = opt->min_seed_len;
	sp.split_len = (int)(opt->min_seed_len * opt->split_factor + .499);   // src/bwamem.c:118
	sp.split_width = opt->split_width;
	if (opt->split_width < 0 || opt->split_width >= 65535) die("split_width %d: the seeding kernel packs re-seed requests into 16 bits", opt->split_width);
	sp.max_mem_intv = (int)opt->max_mem_intv;
	return sp;
}

void c2a_length_tables(const mem_opt_t *opt, int max_len, std::vector<int> &tab)
{
	const int TS = max_len + 2;
	tab.assign(6 * (size_t)TS, 0);
	for (int l = 0; l < TS; ++l) {
		tab[l] = cal_max_gap(opt, l);
		tab[TS + l] = clamp_band(opt, l, 1 << 28, opt->pen_clip5);
		tab[2 * TS + l] = clamp_band(opt, l, 1 << 28, opt->pen_clip3);
		tab[3 * TS + l] = (int)ceil(l * .95);
		tab[4 * TS + l] = (int)floor(.1 * l);
		// mem_flt_chained_seeds returns at once for this length (src/bwamem.c:600-602)
		const double min_l = opt->min_chain_weight ? 1.1f * opt->min_chain_weight : 5.5f * log(l > 0 ? l : 1);
		tab[5 * TS + l] = (l > 0 && min_l > 0.05f * l) ? 1 : 0;
	}
}

void c2a_launch_order(int n, const int *nseeds, int *order)
{
	const int NB = 1024;
	std::vector<int> start(NB + 1, 0);
	for (int i = 0; i < n; ++i) ++start[NB - 1 - std::min(nseeds[i], NB - 1) + 1];
	for (int b = 0; b < NB; ++b) start[b + 1] += start[b];
	for (int i = 0; i < n; ++i) order[start[NB - 1 - std::min(nseeds[i], NB - 1)]++] = i;
}

void c2a_params(const mem_opt_t *opt, int64_t l_pac, int early, C2aParams &cp, ExtParams &ep)
{
	cp.l_pac = l_pac; cp.a = opt->a; cp.w = opt->w; cp.pen_clip5 = opt->pen_clip5; cp.pen_clip3 = opt->pen_clip3;
	cp.early = early;
	memcpy(ep.mat, opt->mat, 25);
	ep.o_del = opt->o_del; ep.e_del = opt->e_del; ep.o_ins = opt->o_ins; ep.e_ins = opt->e_ins; ep.zdrop = opt->zdrop;
}

ChainParams chain_params(const mem_opt_t *opt, int64_t l_pac)
{
	ChainParams kp;
	kp.l_pac = l_pac; kp.w = opt->w; kp.max_chain_gap = opt->max_chain_gap; kp.min_chain_weight = opt->min_chain_weight;
	kp.min_seed_len = opt->min_seed_len; kp.max_chain_extend = opt->max_chain_extend; kp.mask_level = opt->mask_level; kp.drop_ratio = opt->drop_ratio;
	return kp;
}

void contig_table(const bntseq_t *bns, std::vector<int64_t> &ann_off, std::vector<uint8_t> &ann_alt)
{
	ann_off.assign(bns->n_seqs + 1, bns->l_pac);
	ann_alt.assign(bns->n_seqs + 1, 0);
	for (int k = 0; k < bns->n_seqs; ++k) { ann_off[k] = bns->anns[k].offset; ann_alt[k] = bns->anns[k].is_alt ? 1 : 0; }
}

void aln_params(const mem_opt_t *opt, int64_t l_pac, AlnParams &ap, ExtParams &ep)
{
	ap.l_pac = l_pac; ap.a = opt->a; ap.w = opt->w;
	memcpy(ep.mat, opt->mat, 25);
	ep.o_del = opt->o_del; ep.e_del = opt->e_del; ep.o_ins = opt->o_ins; ep.e_ins = opt->e_ins; ep.zdrop = opt->zdrop;
}

void cigar_gap_table(const mem_opt_t *opt, int max_len, std::vector<int> &tab)
{
	tab.resize(max_len + 2);
	for (int l = 0; l <= max_len + 1; ++l) {
		int max_ins = (int)((double)(((l + 1) >> 1) * opt->mat[0] - opt->o_ins) / opt->e_ins + 1.);
		int max_del = (int)((double)(((l + 1) >> 1) * opt->mat[0] - opt->o_del) / opt->e_del + 1.);
		int g = max_ins > max_del ? max_ins : max_del;
		tab[l] = g > 1 ? g : 1;
	}
}

SamParams sam_params(int64_t l_pac, bool has_qual)
{
	SamParams sp;
	sp.l_pac = l_pac; sp.has_qual = has_qual ? 1 : 0;
	sp.rg_len = (int)strnlen(bwa_rg_id, sizeof bwa_rg_id);
	memset(sp.rg, 0, sizeof sp.rg);
	memcpy(sp.rg, bwa_rg_id, (size_t)sp.rg_len);
	return sp;
}

void contig_names(const bntseq_t *bns, std::vector<char> &names, std::vector<int> &name_off)
{
	name_off.assign(bns->n_seqs + 1, 0);
	for (int k = 0; k < bns->n_seqs; ++k) name_off[k + 1] = name_off[k] + (int)strlen(bns->anns[k].name);
	names.resize((size_t)name_off[bns->n_seqs] + 1);
	for (int k = 0; k < bns->n_seqs; ++k) memcpy(names.data() + name_off[k], bns->anns[k].name, (size_t)(name_off[k + 1] - name_off[k]));
}

void queue_aln_sam(void *stream, const mem_opt_t *opt, int64_t l_pac, const ChunkDev &D, const SamParams &sp, const AlnSamJob &J, void *ev_a, void *ev_b)
{
	hipStream_t st = (hipStream_t)stream;
	HIP_OK(hipMemsetAsync(J.d_cnt, 0, 256, st));
	AlnParams ap;
	ExtParams ep;
	aln_params(opt, l_pac, ap, ep);
	if (ev_a) HIP_OK(hipEventRecord((hipEvent_t)ev_a, st));
	if (J.n_req) launch_aln(st, ap, ep, J.n_req, J.d_req, D.d_seq, D.d_off, D.d_pac, D.d_gap, J.d_hdr, J.d_pool, J.d_cnt, J.pool_bytes, D.max_len, D.max_len + 256, J.d_lists);
	if (ev_b) HIP_OK(hipEventRecord((hipEvent_t)ev_b, st));
	if (!J.n_reads) return;
	const int r0 = J.r0, nr = J.n_reads, nu = nr / J.ends;
	if (J.h_desc) HIP_OK(hipMemcpyAsync(J.d_desc + r0, J.h_desc + r0, (size_t)nr * sizeof(SamDesc), hipMemcpyHostToDevice, st));
	HIP_OK(hipMemcpyAsync(J.d_base, J.h_base, (size_t)(nu + 1) * 4, hipMemcpyHostToDevice, st));
	HIP_OK(hipMemsetAsync(J.d_used, 0, 64, st));
	(J.ends == 2 ? launch_sam_emit : launch_sam_emit_se)(st, sp, nr, J.d_desc + r0, J.d_base, J.d_req, J.d_hdr, J.d_pool, D.d_seq, D.d_off + r0, D.d_len + r0, D.d_qual, D.d_names,
	                                                   D.d_noff + r0, D.d_ann_off, D.d_ann_names, D.d_ann_noff, J.d_arena, J.arena_bytes, J.d_used, J.d_ooff, J.d_olen,
	                                                   J.grid_blocks);
}

// band clamp of src/ksw.c:395-407 (host side, double arithmetic as in the reference)
int clamp_band(const mem_opt_t *opt, int qlen, int w, int end_bonus)
{
	int mx = 0;
	for (int i = 0; i < 25; ++i) mx = std::max(mx, (int)opt->mat[i]);
	int max_ins = (int)((double)(qlen * mx + end_bonus - opt->o_ins) / opt->e_ins + 1.);
	int max_del = (int)((double)(qlen * mx + end_bonus - opt->o_del) / opt->e_del + 1.);
	w = std::min(w, std::max(max_ins, 1));
	w = std::min(w, std::max(max_del, 1));
	return w;
}

} // namespace mbw

namespace mbw {
bool pair_params(const mem_opt_t *opt, int64_t l_pac, const mem_pestat_t pes[4], int64_t n_processed, int max_len, PairParams &pp, size_t *n_tab_)
{
	memset(&pp, 0, sizeof pp);
	pp.l_pac = l_pac; pp.a = opt->a; pp.b = opt->b; pp.pen_unpaired = opt->pen_unpaired; pp.min_seed_len = opt->min_seed_len; pp.w = opt->w;
	pp.o_del = opt->o_del; pp.e_del = opt->e_del; pp.o_ins = opt->o_ins; pp.e_ins = opt->e_ins;
	pp.max_chain_gap = opt->max_chain_gap; pp.mask_level_redun = opt->mask_level_redun; pp.mask_level = opt->mask_level;
	pp.XA_drop_ratio = opt->XA_drop_ratio; pp.T = opt->T; pp.max_matesw = opt->max_matesw; pp.id0 = (uint64_t)(n_processed >> 1);
	for (int v = 0; v < 40; ++v) pp.lnq[v] = (int)(4.343 * log(v + 1) + .499);
	pp.no_rescue = ((opt->flag & MEM_F_NO_RESCUE) || opt->max_matesw <= 0) ? 1 : 0;
	bool usable = true;
	size_t n_tab = 0;
	for (int d = 0; d < 4; ++d) {
		pp.low[d] = pes[d].low; pp.high[d] = pes[d].high; pp.failed[d] = pes[d].failed ? 1 : 0;
		pp.tab_off[d] = (int)n_tab;
		if (!pes[d].failed) {
			// (a degenerate distribution — std 0, as a user's -I can give — makes the pair score NaN / infinite for some distances,
			// and the conversion of those to int is the one place where the host's and the device's arithmetic differ: host path)
			if (!(pes[d].std > 0) || !std::isfinite(pes[d].avg) || !std::isfinite(pes[d].std)) usable = false;
			if (pes[d].high < pes[d].low || (int64_t)pes[d].high - pes[d].low > (1 << 20)) usable = false;
			else n_tab += (size_t)(pes[d].high - pes[d].low + 1);
		}
	}
	pp.ltab_n = 4 * max_len + 256;
	pp.max_XA_hits = std::min(opt->max_XA_hits, opt->max_XA_hits_alt);
	*n_tab_ = n_tab;
	return usable;
}
void pair_tables(const mem_opt_t *opt, const mem_pestat_t pes[4], const PairParams &pp, size_t n_tab, double *tab)
{
	for (int d = 0; d < 4; ++d)
		if (!pes[d].failed)
			for (int64_t dist = pes[d].low; dist <= pes[d].high; ++dist) {   // src/bwamem_pair.c:218-219, the double part of q
				const double ns = (dist - pes[d].avg) / pes[d].std;
				tab[pp.tab_off[d] + (dist - pes[d].low)] = .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * opt->a;
			}
	double *ltab = tab + n_tab;
	ltab[0] = 1.;
	for (int l = 1; l < pp.ltab_n; ++l) ltab[l] = l < opt->mapQ_coef_len ? 1. : opt->mapQ_coef_fac / log(l);   // src/bwamem.c:964
}
void se_params(const mem_opt_t *opt, int64_t l_pac, int64_t n_processed, int max_len, PairParams &pp, mem_pestat_t pes[4])
{
	memset(pes, 0, 4 * sizeof(mem_pestat_t));
	for (int d = 0; d < 4; ++d) pes[d].failed = 1;
	size_t n_tab = 0;
	pair_params(opt, l_pac, pes, n_processed, max_len, pp, &n_tab);   // (no orientation to tabulate: always usable, n_tab = 0)
	pp.id0 = (uint64_t)n_processed;   // NOT pair_params' n_processed >> 1: the hash id of a single-end read is n_processed + i, of a pair (n_processed >> 1) + i
	pp.no_rescue = 1;
}
} // namespace mbw

// Stage entry of se_simple_kernel (se_kernel.hip) for parity tests: n_reads single-end reads given by their regions as they stand after
// phase 1 (regs: PR_MAXREG DevReg records per read, n_regs per read); status[i] = 1: decided — desc[i] (SamDesc) and req[i] (AlnReq) are
// what mem_reg2sam reports with one line; else the code of the test that sent the read to the host (device.h: SE_HOST_*).
extern "C" int mi355x_se_batch(const mem_opt_t *opt, const bntseq_t *bns, int64_t n_processed, int n_reads, const void *regs, const int *n_regs,
                               int max_len, uint8_t *status, void *desc, void *req)
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n_reads <= 0) return 0;
	if (max_len <= 0) die("mi355x_se_batch: max_len must be positive");
	PairParams pp;
	mem_pestat_t pes[4];
	se_params(opt, bns->l_pac, n_processed, max_len, pp, pes);
	std::vector<double> tab((size_t)pp.ltab_n);
	pair_tables(opt, pes, pp, 0, tab.data());
	std::vector<int64_t> ann_off;
	std::vector<uint8_t> ann_alt, ok((size_t)n_reads, 1);
	contig_table(bns, ann_off, ann_alt);
	const size_t n = (size_t)n_reads;
	const DevReg *hr = (const DevReg *)regs;
	for (size_t i = 0; i < n; ++i)   // nothing the kernel indexes with may point outside what is uploaded
		for (int j = 0; j < n_regs[i] && j < PR_MAXREG; ++j)
			if (hr[i * PR_MAXREG + j].rid < 0 || hr[i * PR_MAXREG + j].rid >= bns->n_seqs) die("mi355x_se_batch: bad contig in region %d of read %zu", j, i);
	DevReg *d_first; int *d_nf; uint8_t *d_ok, *d_aa, *d_st; double *d_tab; AlnReq *d_rq; SamDesc *d_ds;
	HIP_OK(hipMalloc(&d_first, n * PR_MAXREG * sizeof(DevReg))); HIP_OK(hipMalloc(&d_nf, n * 4)); HIP_OK(hipMalloc(&d_ok, n));
	HIP_OK(hipMalloc(&d_aa, ann_alt.size())); HIP_OK(hipMalloc(&d_st, n)); HIP_OK(hipMalloc(&d_tab, tab.size() * 8));
	HIP_OK(hipMalloc(&d_rq, n * sizeof(AlnReq))); HIP_OK(hipMalloc(&d_ds, n * sizeof(SamDesc)));
	HIP_OK(hipMemcpy(d_first, regs, n * PR_MAXREG * sizeof(DevReg), hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_nf, n_regs, n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_ok, ok.data(), n, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_aa, ann_alt.data(), ann_alt.size(), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
	launch_se_simple(0, pp, n_reads, d_first, d_nf, d_ok, d_aa, d_tab, d_st, d_rq, d_ds);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	HIP_OK(hipMemcpy(status, d_st, n, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(desc, d_ds, n * sizeof(SamDesc), hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(req, d_rq, n * sizeof(AlnReq), hipMemcpyDeviceToHost));
	(void)hipFree(d_first); (void)hipFree(d_nf); (void)hipFree(d_ok); (void)hipFree(d_aa); (void)hipFree(d_st); (void)hipFree(d_tab);
	(void)hipFree(d_rq); (void)hipFree(d_ds);
	return 0;
}

// Stage entry of pair_simple_kernel (pair_kernel.hip) for parity tests: n_pairs pairs given by the regions of their two ends
// (regs: PR_MAXREG DevReg records per read, n_regs per read) as they stand after phase 1; status[k] = 1: decided — desc[2k], desc[2k+1]
// (SamDesc) and req[2k], req[2k+1] (AlnReq) are what mem_sam_pe's paired branch reports; else the code of the test that sent the pair to
// the host.  Returns 0, or -1 when the insert-size statistics are not usable by the kernel.
extern "C" int mi355x_pair_maxreg(void) { return PR_MAXREG; }
extern "C" int mi355x_pair_batch(const mem_opt_t *opt, const bntseq_t *bns, const mem_pestat_t pes[4], int64_t n_processed, int n_pairs,
                                 const void *regs, const int *n_regs, int max_len, uint8_t *status, void *desc, void *req)
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n_pairs <= 0) return 0;
	PairParams pp;
	size_t n_tab = 0;
	if (!pair_params(opt, bns->l_pac, pes, n_processed, max_len, pp, &n_tab)) return -1;
	std::vector<double> tab(n_tab + (size_t)pp.ltab_n);
	pair_tables(opt, pes, pp, n_tab, tab.data());
	std::vector<int64_t> ann_off;
	std::vector<uint8_t> ann_alt, ok((size_t)n_pairs, 1);
	contig_table(bns, ann_off, ann_alt);
	const size_t n = (size_t)2 * n_pairs;
	DevReg *d_first; int *d_nf; uint8_t *d_ok, *d_aa, *d_st; int64_t *d_ao; double *d_tab; AlnReq *d_rq; SamDesc *d_ds;
	HIP_OK(hipMalloc(&d_first, n * PR_MAXREG * sizeof(DevReg))); HIP_OK(hipMalloc(&d_nf, n * 4)); HIP_OK(hipMalloc(&d_ok, n_pairs));
	HIP_OK(hipMalloc(&d_aa, ann_alt.size())); HIP_OK(hipMalloc(&d_st, n_pairs)); HIP_OK(hipMalloc(&d_ao, ann_off.size() * 8));
	HIP_OK(hipMalloc(&d_tab, tab.size() * 8)); HIP_OK(hipMalloc(&d_rq, n * sizeof(AlnReq))); HIP_OK(hipMalloc(&d_ds, n * sizeof(SamDesc)));
	HIP_OK(hipMemcpy(d_first, regs, n * PR_MAXREG * sizeof(DevReg), hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_nf, n_regs, n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_ok, ok.data(), n_pairs, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_aa, ann_alt.data(), ann_alt.size(), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_ao, ann_off.data(), ann_off.size() * 8, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
	launch_pair_simple(0, pp, n_pairs, d_first, d_nf, d_ok, d_ao, d_aa, d_tab, d_tab + n_tab, d_st, d_rq, d_ds);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	HIP_OK(hipMemcpy(status, d_st, n_pairs, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(desc, d_ds, n * sizeof(SamDesc), hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(req, d_rq, n * sizeof(AlnReq), hipMemcpyDeviceToHost));
	(void)hipFree(d_first); (void)hipFree(d_nf); (void)hipFree(d_ok); (void)hipFree(d_aa); (void)hipFree(d_st); (void)hipFree(d_ao); (void)hipFree(d_tab);
	(void)hipFree(d_rq); (void)hipFree(d_ds);
	return 0;
}

// Stage entry of pair_wave_kernel (pair_wave_kernel.hip) for parity tests.  It runs the pipeline's own sequence — the host lists the
// mate-rescue windows with their tags (sam_pe_msw_collect_tagged), launch_msw aligns them, pair_wave_kernel replays mem_sam_pe — on
// n_pairs pairs given by their reads (nt4 codes, off[2 n_pairs + 1]) and both ends' regions as they stand after mem_sort_dedup_patch
// (regs: DevReg records back to back, reg_off[2 n_pairs + 1]).  A pair whose lists are not fixed points of the redundancy pass, hold more
// than PW_MAXREG regions or an ALT hit, or that has no region at all, is not handed to the kernel (status 0).  status[k] = 1: decided —
// desc[2k], desc[2k + 1] (SamDesc) and req[2k], req[2k + 1] (AlnReq) are what mem_sam_pe's paired branch reports; else the code of the
// test that left the pair to the host.  *n_align = mate-rescue alignments run.  Returns 0, or -1 when the insert-size statistics are not
// usable by the kernel.
// xa_req given: XA on (mi355x_pair_wave_xa_batch) — status PW_DECIDED_XA: decided with an XA tag on a record; xa_cnt[2k + e] entries of
// end e, their requests at xa_req[(2k + e) * PW_XA_CAP ..] (AlnReq, pad = the entry's contig), the counts also in desc[].flag bits 16-19.
extern "C" int mi355x_pair_wave_maxreg(void) { return PW_MAXREG; }
extern "C" int mi355x_pair_wave_xa_cap(void) { return PW_XA_CAP; }
static int pair_wave_batch(const char *who, const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], int64_t n_processed,
                           int n_pairs, const uint8_t *reads, const int64_t *off, const void *regs, const int *reg_off, uint8_t *status,
                           void *desc, void *req, int *n_align, void *xa_req, uint8_t *xa_cnt)
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n_align) *n_align = 0;
	if (n_pairs <= 0) return 0;
	const int n_reads = 2 * n_pairs;
	memset(status, 0, (size_t)n_pairs);
	memset(desc, 0xff, (size_t)n_reads * sizeof(SamDesc));
	memset(req, 0xff, (size_t)n_reads * sizeof(AlnReq));
	if (xa_req) { memset(xa_req, 0xff, (size_t)n_reads * PW_XA_CAP * sizeof(AlnReq)); memset(xa_cnt, 0, (size_t)n_reads); }
	// (the calls whose pairs are all the host's, as for pair_simple_kernel: -P, -a, -V, -5, mapQ_coef_len 0)
	if ((opt->flag & (MEM_F_NOPAIRING | MEM_F_ALL | MEM_F_REF_HDR | MEM_F_PRIMARY5)) || !(opt->mapQ_coef_len > 0)) return 0;
	const int64_t l_pac = bns->l_pac;
	std::vector<int64_t> slot(n_reads + 1);
	std::vector<int> lens(n_reads);
	int max_len = 1;
	slot[0] = 0;
	for (int i = 0; i < n_reads; ++i) {
		lens[i] = (int)(off[i + 1] - off[i]);
		slot[i + 1] = slot[i] + ((lens[i] + 15) & ~15);
		max_len = std::max(max_len, lens[i]);
	}
	if ((int64_t)max_len * opt->a >= 8192 || msw_lds_bytes(max_len) > 160 * 1024) die("mate-rescue kernel: reads too long for the device path");
	PairParams pp;
	size_t n_tab = 0;
	if (!pair_params(opt, l_pac, pes, n_processed, max_len, pp, &n_tab)) return -1;
	std::vector<double> tab(n_tab + (size_t)pp.ltab_n);
	pair_tables(opt, pes, pp, n_tab, tab.data());
	std::vector<int64_t> ann_off;
	std::vector<uint8_t> ann_alt;
	contig_table(bns, ann_off, ann_alt);
	// ---- the host's part: eligibility, windows, tags ----
	const DevReg *hr = (const DevReg *)regs;
	std::vector<int> work, loff(1, 0), toff;
	std::vector<unsigned> mfirst;
	std::vector<DevReg> lists;
	std::vector<MswReqH> mreq;
	std::vector<int16_t> tags;
	std::vector<bseq1_t> s(2);
	for (int k = 0; k < n_pairs; ++k) {
		status[k] = 0;
		HRegV a[2];
		bool ok = true;
		for (int e = 0; e < 2 && ok; ++e) {
			for (int j = reg_off[2 * k + e]; j < reg_off[2 * k + e + 1]; ++j) {
				const DevReg &d = hr[j];
				if (d.rid < 0 || d.rid >= bns->n_seqs) die("%s: bad contig in a region of pair %d", who, k);
				HReg h;
				h.rb = d.rb; h.re = d.re; h.qb = d.qb; h.qe = d.qe; h.rid = d.rid; h.score = d.score; h.truesc = d.truesc; h.w = d.w;
				h.seedcov = d.seedcov; h.seedlen0 = d.seedlen0; h.frac_rep = d.frac_rep; h.secondary = -1; h.is_alt = bns->anns[d.rid].is_alt;
				a[e].push_back(h);
			}
			// settled = another redundancy pass without patching returns the list as it is
			HRegV c;
			for (size_t j = 0; j < a[e].size(); ++j) c.push_back(a[e][j]);
			sort_dedup_patch(opt, 0, 0, 0, c);
			ok = c.size() == a[e].size() && c.settled;
			for (size_t j = 0; j < c.size() && ok; ++j) ok = c[j].rb == a[e][j].rb && c[j].re == a[e][j].re && c[j].qb == a[e][j].qb && c[j].score == a[e][j].score;
			a[e].settled = ok;
		}
		if (!ok || !pair_wave_eligible(a, PW_MAXREG)) continue;
		s[0].l_seq = lens[2 * k]; s[1].l_seq = lens[2 * k + 1];
		work.push_back(k);
		mfirst.push_back((unsigned)mreq.size());
		toff.push_back((int)tags.size());
		sam_pe_msw_collect_tagged(opt, bns, pes, s.data(), a, 2 * k, 4096, mreq, tags);
		for (int e = 0; e < 2; ++e) {
			lists.insert(lists.end(), hr + reg_off[2 * k + e], hr + reg_off[2 * k + e + 1]);
			loff.push_back((int)lists.size());
		}
	}
	const int n_work = (int)work.size();
	toff.push_back((int)tags.size());
	const size_t n_mreq = mreq.size();
	if (n_align) *n_align = (int)n_mreq;
	if (n_work == 0) return 0;
	// ---- device ----
	hipStream_t st = 0;
	std::vector<uint8_t> flat(slot[n_reads] + 16, 4);
	for (int i = 0; i < n_reads; ++i) memcpy(flat.data() + slot[i], reads + off[i], lens[i]);
	int max_t = 1;
	for (size_t i = 0; i < n_mreq; ++i) max_t = std::max(max_t, (int)(mreq[i].re - mreq[i].rb));
	std::vector<void *> owned;
	auto up = [&](const void *h, size_t bytes) -> void * {
		void *d = nullptr;
		HIP_OK(hipMalloc(&d, bytes + 64));
		owned.push_back(d);
		if (h && bytes) HIP_OK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
		return d;
	};
	uint8_t *d_seq = (uint8_t *)up(flat.data(), flat.size());
	uint8_t *d_pac = (uint8_t *)up(pac, (size_t)(l_pac / 4 + 1));
	int64_t *d_off = (int64_t *)up(slot.data(), (size_t)(n_reads + 1) * 8);
	int *d_len = (int *)up(lens.data(), (size_t)n_reads * 4);
	MswReq *d_mreq = (MswReq *)up(mreq.data(), n_mreq * sizeof(MswReq));
	MswRes *d_mres = (MswRes *)up(nullptr, n_mreq * sizeof(MswRes));
	if (n_mreq) {
		uint16_t *d_rows = (uint16_t *)up(nullptr, n_mreq * (size_t)max_t * 2);
		std::vector<int> h_list(2 * n_mreq + 16);
		int *d_list = (int *)up(nullptr, (2 * n_mreq + 16) * sizeof(int));
		int *d_tail = (int *)up(nullptr, msw_tail_ints(n_mreq) * sizeof(int));
		launch_msw(st, msw_params(opt, l_pac), (int)n_mreq, d_mreq, d_seq, d_off, d_len, d_pac, d_mres, d_rows, max_len, (const MswReq *)mreq.data(), lens.data(),
		           h_list.data(), d_list, d_tail);
		HIP_OK(hipStreamSynchronize(st));   // (h_list is read by the copy queued in launch_msw)
	}
	int *d_work = (int *)up(work.data(), (size_t)n_work * 4);
	DevReg *d_lists = (DevReg *)up(lists.data(), lists.size() * sizeof(DevReg));
	int *d_loff = (int *)up(loff.data(), loff.size() * 4);
	unsigned *d_mfirst = (unsigned *)up(mfirst.data(), mfirst.size() * 4);
	short *d_tags = (short *)up(tags.data(), tags.size() * 2);
	int *d_toff = (int *)up(toff.data(), toff.size() * 4);
	int64_t *d_ao = (int64_t *)up(ann_off.data(), ann_off.size() * 8);
	double *d_tab = (double *)up(tab.data(), tab.size() * 8);
	uint8_t *d_ws = (uint8_t *)up(nullptr, (size_t)n_work);
	AlnReq *d_rq = (AlnReq *)up(nullptr, (size_t)2 * n_work * sizeof(AlnReq));
	SamDesc *d_ds = (SamDesc *)up(nullptr, (size_t)2 * n_work * sizeof(SamDesc));
	AlnReq *d_xr = xa_req ? (AlnReq *)up(nullptr, (size_t)2 * n_work * PW_XA_CAP * sizeof(AlnReq)) : nullptr;
	uint8_t *d_xc = xa_req ? (uint8_t *)up(nullptr, (size_t)2 * n_work) : nullptr;
	HIP_OK(hipMemset(d_ws, 0, (size_t)n_work));
	if (d_xc) HIP_OK(hipMemset(d_xc, 0, (size_t)2 * n_work));
	launch_pair_wave(st, pp, n_work, d_work, d_lists, d_loff, d_len, d_mreq, d_mres, d_mfirst, d_tags, d_toff, d_ao, d_tab, d_tab + n_tab, d_ws, d_rq, d_ds,
	                 d_xr, d_xc);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	std::vector<uint8_t> ws((size_t)n_work);
	HIP_OK(hipMemcpy(ws.data(), d_ws, (size_t)n_work, hipMemcpyDeviceToHost));
	std::vector<SamDesc> w_ds((size_t)2 * n_work);
	std::vector<AlnReq> w_rq((size_t)2 * n_work);
	HIP_OK(hipMemcpy(w_ds.data(), d_ds, w_ds.size() * sizeof(SamDesc), hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(w_rq.data(), d_rq, w_rq.size() * sizeof(AlnReq), hipMemcpyDeviceToHost));
	std::vector<AlnReq> w_xr(xa_req ? (size_t)2 * n_work * PW_XA_CAP : 0);
	std::vector<uint8_t> w_xc(xa_req ? (size_t)2 * n_work : 0);
	if (xa_req) {
		HIP_OK(hipMemcpy(w_xr.data(), d_xr, w_xr.size() * sizeof(AlnReq), hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy(w_xc.data(), d_xc, w_xc.size(), hipMemcpyDeviceToHost));
	}
	for (int t = 0; t < n_work; ++t) {
		status[work[t]] = ws[t];
		if (ws[t] != 1 && ws[t] != PW_DECIDED_XA) continue;
		for (int e = 0; e < 2; ++e) { ((SamDesc *)desc)[2 * work[t] + e] = w_ds[2 * t + e]; ((AlnReq *)req)[2 * work[t] + e] = w_rq[2 * t + e]; }
		if (ws[t] != PW_DECIDED_XA) continue;
		for (int e = 0; e < 2; ++e) {
			const int c = std::min<int>(w_xc[2 * t + e], PW_XA_CAP);
			xa_cnt[2 * work[t] + e] = (uint8_t)c;
			memcpy((AlnReq *)xa_req + (size_t)(2 * work[t] + e) * PW_XA_CAP, &w_xr[(size_t)(2 * t + e) * PW_XA_CAP], (size_t)c * sizeof(AlnReq));
		}
	}
	for (void *d : owned) (void)hipFree(d);
	return 0;
}
extern "C" int mi355x_pair_wave_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], int64_t n_processed,
                                      int n_pairs, const uint8_t *reads, const int64_t *off, const void *regs, const int *reg_off, uint8_t *status,
                                      void *desc, void *req, int *n_align)
{
	return pair_wave_batch("mi355x_pair_wave_batch", opt, bns, pac, pes, n_processed, n_pairs, reads, off, regs, reg_off, status, desc, req, n_align, nullptr,
	                       nullptr);
}
extern "C" int mi355x_pair_wave_xa_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], int64_t n_processed,
                                         int n_pairs, const uint8_t *reads, const int64_t *off, const void *regs, const int *reg_off, uint8_t *status,
                                         void *desc, void *req, int *n_align, void *xa_req, uint8_t *xa_cnt)
{
	if (!xa_req || !xa_cnt) die("mi355x_pair_wave_xa_batch: no room for the XA requests");
	return pair_wave_batch("mi355x_pair_wave_xa_batch", opt, bns, pac, pes, n_processed, n_pairs, reads, off, regs, reg_off, status, desc, req, n_align, xa_req,
	                       xa_cnt);
}

extern "C" int mi355x_smem_batch(const mem_opt_t *opt, int n, const uint8_t *seqs, const int64_t *off, int cap,
                                 uint64_t *intv_out, int *n_out, double *kernel_ms, uint64_t *algo_bytes)
{
	need_index();
	if (n <= 0) return 0;
	hipStream_t st = 0;
	int max_len = 0;
	std::vector<int64_t> poff(n + 1);   // 16-byte aligned slots, as the kernel expects
	std::vector<int> lens(n);
	poff[0] = 0;
	for (int i = 0; i < n; ++i) {
		lens[i] = (int)(off[i + 1] - off[i]);
		max_len = std::max(max_len, lens[i]);
		poff[i + 1] = poff[i] + ((lens[i] + 15) & ~15);
	}
	size_t total = off[n];
	std::vector<uint8_t> packed(poff[n] + 16, 0);
	for (int i = 0; i < n; ++i) memcpy(packed.data() + poff[i], seqs + off[i], lens[i]);
	uint8_t *d_seq; int64_t *d_off; uint64_t *d_out; int *d_nout, *d_len; unsigned long long *d_cnt; void *d_scr;
	HIP_OK(hipMalloc(&d_seq, packed.size()));
	HIP_OK(hipMalloc(&d_len, (size_t)n * 4));
	HIP_OK(hipMalloc(&d_off, (size_t)(n + 1) * 8));
	HIP_OK(hipMalloc(&d_out, (size_t)n * cap * 32));
	HIP_OK(hipMalloc(&d_nout, (size_t)n * 4));
	HIP_OK(hipMalloc(&d_cnt, 256));
	size_t per_quad = 0;
	int n_quads = smem_grid_quads(max_len, &per_quad);
	HIP_OK(hipMalloc(&d_scr, per_quad * n_quads));
	HIP_OK(hipMemcpy(d_seq, packed.data(), packed.size(), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_off, poff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_len, lens.data(), (size_t)n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemset(d_cnt, 0, 256));
	HIP_OK(hipMemset(d_nout, 0, (size_t)n * 4));
	Timer tm;
	tm.start(st);
	const char *ce = getenv("MPIBWA_SMEM_COUNT");   // "0": the production variant of passes 1-2 (no block counting; *algo_bytes = 0)
	const bool count_blocks = !(ce && atoi(ce) == 0);
	launch_smem(st, g_idx.fm, smem_params(opt), n, d_seq, d_off, d_len, cap, d_out, d_nout, max_len, d_cnt, d_scr, per_quad, n_quads, count_blocks);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	unsigned long long cnt[32];
	HIP_OK(hipMemcpy(cnt, d_cnt, 256, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(n_out, d_nout, (size_t)n * 4, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(intv_out, d_out, (size_t)n * cap * 32, hipMemcpyDeviceToHost));
	(void)hipFree(d_seq); (void)hipFree(d_off); (void)hipFree(d_out); (void)hipFree(d_nout); (void)hipFree(d_cnt);
	(void)hipFree(d_scr); (void)hipFree(d_len);
	// order by info (the reference sorts with an unstable introsort keyed on info only, src/bwamem.c:161;
	// equal keys are identical records, so any order of ties is the same byte sequence)
	uint64_t n_intv = 0;
	for (int i = 0; i < n; ++i) {
		int m = std::min(n_out[i], cap);
		Intv *a = (Intv *)(intv_out + (size_t)i * cap * 4);
		std::sort(a, a + m, [](const Intv &x, const Intv &y) { return x.info < y.info; });
		n_intv += m;
	}
	if (kernel_ms) *kernel_ms = ms;
	if (algo_bytes) *algo_bytes = count_blocks ? cnt[1] * 64 + total + n_intv * 32 : 0;   // 64 B per occ block + read + output
	return cnt[2] ? -1 : 0;
}

// dense != 0: answer from the expanded table (fails if it is absent); dense == 0: LF walk on the sampled SA
extern "C" int mi355x_sa_batch2(int n, const uint64_t *k, uint64_t *sa_out, double *kernel_ms, int dense)
{
	need_index();
	if (!dense) return mi355x_sa_batch(n, k, sa_out, kernel_ms, nullptr);
	if (!g_idx.fm.sa_full) return -1;
	if (n <= 0) return 0;
	uint64_t *d_k, *d_o;
	HIP_OK(hipMalloc(&d_k, (size_t)n * 8)); HIP_OK(hipMalloc(&d_o, (size_t)n * 8));
	HIP_OK(hipMemcpy(d_k, k, (size_t)n * 8, hipMemcpyHostToDevice));
	Timer tm;
	tm.start(0);
	launch_sa_dense(0, g_idx.fm, n, d_k, d_o);
	double ms = tm.stop(0);
	HIP_OK(hipGetLastError());
	HIP_OK(hipMemcpy(sa_out, d_o, (size_t)n * 8, hipMemcpyDeviceToHost));
	(void)hipFree(d_k); (void)hipFree(d_o);
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}
extern "C" double mi355x_sa_dense_info(size_t *bytes) { if (bytes) *bytes = g_idx.sa_full_bytes; return g_idx.sa_expand_ms; }

extern "C" int mi355x_sa_batch(int n, const uint64_t *k, uint64_t *sa_out, double *kernel_ms, uint64_t *algo_bytes)
{
	need_index();
	if (n <= 0) return 0;
	hipStream_t st = 0;
	uint64_t *d_k, *d_o; unsigned long long *d_cnt;
	HIP_OK(hipMalloc(&d_k, (size_t)n * 8));
	HIP_OK(hipMalloc(&d_o, (size_t)n * 8));
	HIP_OK(hipMalloc(&d_cnt, 64));
	HIP_OK(hipMemcpy(d_k, k, (size_t)n * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemset(d_cnt, 0, 64));
	Timer tm;
	tm.start(st);
	launch_sa(st, g_idx.fm, n, d_k, d_o, d_cnt);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	unsigned long long cnt[8];
	HIP_OK(hipMemcpy(cnt, d_cnt, 64, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(sa_out, d_o, (size_t)n * 8, hipMemcpyDeviceToHost));
	(void)hipFree(d_k); (void)hipFree(d_o); (void)hipFree(d_cnt);
	if (kernel_ms) *kernel_ms = ms;
	if (algo_bytes) *algo_bytes = cnt[1] * 64 + (uint64_t)n * 8;   // 64 B per LF step + the sampled SA word
	return 0;
}

extern "C" int mi355x_extend_batch(const mem_opt_t *opt, int n, const uint8_t *q, const int64_t *qoff, const uint8_t *t,
                                   const int64_t *toff, const int *w, const int *h0, const int *end_bonus, int *out6,
                                   double *kernel_ms, uint64_t *cells)
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n <= 0) return 0;
	hipStream_t st = 0;
	std::vector<int> wc(n);
	int max_qlen = 0;
	for (int i = 0; i < n; ++i) {
		int ql = (int)(qoff[i + 1] - qoff[i]);
		max_qlen = std::max(max_qlen, ql);
		wc[i] = clamp_band(opt, ql, w[i], end_bonus[i]);
	}
	uint8_t *d_q, *d_t; int64_t *d_qo, *d_to; int *d_w, *d_h0, *d_out; unsigned long long *d_cells;
	HIP_OK(hipMalloc(&d_q, qoff[n] + 16)); HIP_OK(hipMalloc(&d_t, toff[n] + 16));
	HIP_OK(hipMalloc(&d_qo, (size_t)(n + 1) * 8)); HIP_OK(hipMalloc(&d_to, (size_t)(n + 1) * 8));
	HIP_OK(hipMalloc(&d_w, (size_t)n * 4)); HIP_OK(hipMalloc(&d_h0, (size_t)n * 4));
	HIP_OK(hipMalloc(&d_out, (size_t)n * 24)); HIP_OK(hipMalloc(&d_cells, 8));
	HIP_OK(hipMemcpy(d_q, q, qoff[n], hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_t, t, toff[n], hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_qo, qoff, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_to, toff, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_w, wc.data(), (size_t)n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_h0, h0, (size_t)n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemset(d_cells, 0, 8));
	ExtParams ep;
	memcpy(ep.mat, opt->mat, 25);
	ep.o_del = opt->o_del; ep.e_del = opt->e_del; ep.o_ins = opt->o_ins; ep.e_ins = opt->e_ins; ep.zdrop = opt->zdrop;
	Timer tm;
	tm.start(st);
	launch_extend(st, ep, n, d_q, d_qo, d_t, d_to, d_w, d_h0, nullptr, d_out, d_cells, max_qlen);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	unsigned long long c = 0;
	HIP_OK(hipMemcpy(&c, d_cells, 8, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(out6, d_out, (size_t)n * 24, hipMemcpyDeviceToHost));
	(void)hipFree(d_q); (void)hipFree(d_t); (void)hipFree(d_qo); (void)hipFree(d_to); (void)hipFree(d_w);
	(void)hipFree(d_h0); (void)hipFree(d_out); (void)hipFree(d_cells);
	if (kernel_ms) *kernel_ms = ms;
	if (cells) *cells = c;
	return 0;
}

extern "C" int mi355x_extend_batch2(const mem_opt_t *opt, int n, const uint8_t *q, const int64_t *qoff, const uint8_t *t,
                                    const int64_t *toff, const int *w, const int *h0, const int *end_bonus, const int *early,
                                    const int *clip, int *out6, uint64_t *cells, double *kernel_ms)
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n <= 0) return 0;
	hipStream_t st = 0;
	std::vector<int> wc(n);
	int max_qlen = 0;
	for (int i = 0; i < n; ++i) {
		int ql = (int)(qoff[i + 1] - qoff[i]);
		max_qlen = std::max(max_qlen, ql);
		wc[i] = clamp_band(opt, ql, w[i], end_bonus[i]);
	}
	uint8_t *d_q, *d_t; int64_t *d_qo, *d_to; int *d_w, *d_h0, *d_early, *d_clip, *d_out; unsigned long long *d_cells;
	HIP_OK(hipMalloc(&d_q, qoff[n] + 16)); HIP_OK(hipMalloc(&d_t, toff[n] + 16));
	HIP_OK(hipMalloc(&d_qo, (size_t)(n + 1) * 8)); HIP_OK(hipMalloc(&d_to, (size_t)(n + 1) * 8));
	HIP_OK(hipMalloc(&d_w, (size_t)n * 4)); HIP_OK(hipMalloc(&d_h0, (size_t)n * 4));
	HIP_OK(hipMalloc(&d_early, (size_t)n * 4)); HIP_OK(hipMalloc(&d_clip, (size_t)n * 4));
	HIP_OK(hipMalloc(&d_out, (size_t)n * 24)); HIP_OK(hipMalloc(&d_cells, (size_t)n * 8));
	HIP_OK(hipMemcpy(d_q, q, qoff[n], hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_t, t, toff[n], hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_qo, qoff, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_to, toff, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_w, wc.data(), (size_t)n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_h0, h0, (size_t)n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_early, early, (size_t)n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_clip, clip, (size_t)n * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemset(d_cells, 0, (size_t)n * 8));
	ExtParams ep;
	memcpy(ep.mat, opt->mat, 25);
	ep.o_del = opt->o_del; ep.e_del = opt->e_del; ep.o_ins = opt->o_ins; ep.e_ins = opt->e_ins; ep.zdrop = opt->zdrop;
	Timer tm;
	tm.start(st);
	launch_extend2(st, ep, n, d_q, d_qo, d_t, d_to, d_w, d_h0, d_early, d_clip, d_out, d_cells, max_qlen);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	HIP_OK(hipMemcpy(cells, d_cells, (size_t)n * 8, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(out6, d_out, (size_t)n * 24, hipMemcpyDeviceToHost));
	(void)hipFree(d_q); (void)hipFree(d_t); (void)hipFree(d_qo); (void)hipFree(d_to); (void)hipFree(d_w);
	(void)hipFree(d_h0); (void)hipFree(d_early); (void)hipFree(d_clip); (void)hipFree(d_out); (void)hipFree(d_cells);
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}

namespace mbw {
MswParams msw_params(const mem_opt_t *opt, int64_t l_pac)
{
	MswParams P;
	P.l_pac = l_pac;
	int8_t mn = 127, mx = 0;   // initial values of the reference's scan (src/ksw.c:83-87)
	for (int i = 0; i < 25; ++i) {
		if (opt->mat[i] < mn) mn = opt->mat[i];
		if (opt->mat[i] > mx) mx = opt->mat[i];
	}
	for (int t = 0; t < 4; ++t) {
		P.slo[t] = 0;
		for (int q = 0; q < 4; ++q) P.slo[t] |= (uint32_t)(uint8_t)opt->mat[t * 5 + q] << (8 * q);
		P.s4[t] = opt->mat[t * 5 + 4];
	}
	P.o_del = opt->o_del; P.e_del = opt->e_del; P.o_ins = opt->o_ins; P.e_ins = opt->e_ins;
	P.a = opt->a; P.min_seed_len = opt->min_seed_len;
	P.max_sc = mx > 0 ? mx : 1;
	P.shift = (uint8_t)(256 - (uint8_t)mn);
	return P;
}
}

// Stage-level entry point of the mate-rescue alignment (tests, micro-benchmarks): n_req windows [rb,re) of the packed
// reference `pac` (doubled coordinate, 2 bits per base, l_pac bases) against reads of a batch given as nt4 codes.
// out8 per request: score, te, qe, score2, te2, tb, qb, flags — kswr_t of ksw_align2 with mem_matesw's flags.
extern "C" int mi355x_matesw_batch(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, int n_reads, const uint8_t *reads, const int64_t *off,
                                   int n_req, const int64_t *rb, const int64_t *re, const int *read, const int *is_rev, int *out8,
                                   double *kernel_ms)
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n_req <= 0) return 0;
	hipStream_t st = 0;
	// reads go into 16-byte slots as in the pipeline
	std::vector<int64_t> slot(n_reads + 1);
	std::vector<int> lens(n_reads);
	int max_len = 0;
	slot[0] = 0;
	for (int i = 0; i < n_reads; ++i) {
		lens[i] = (int)(off[i + 1] - off[i]);
		slot[i + 1] = slot[i] + ((lens[i] + 15) & ~15);
		max_len = std::max(max_len, lens[i]);
	}
	if ((int64_t)max_len * opt->a >= 8192 || msw_lds_bytes(max_len) > 160 * 1024) die("mate-rescue kernel: reads too long for the device path");
	std::vector<uint8_t> flat(slot[n_reads] + 16, 4);
	for (int i = 0; i < n_reads; ++i) memcpy(flat.data() + slot[i], reads + off[i], lens[i]);
	std::vector<MswReq> rq(n_req);
	int max_t = 1;
	for (int i = 0; i < n_req; ++i) {
		rq[i].rb = rb[i]; rq[i].re = re[i]; rq[i].read = read[i]; rq[i].is_rev = is_rev[i];
		if (re[i] < rb[i] || re[i] > 2 * l_pac || rb[i] < 0 || read[i] < 0 || read[i] >= n_reads) die("mi355x_matesw_batch: bad request %d", i);
		max_t = std::max(max_t, (int)(re[i] - rb[i]));
	}
	uint8_t *d_seq, *d_pac; int64_t *d_off; int *d_len; MswReq *d_req; MswRes *d_res; uint16_t *d_rows;
	HIP_OK(hipMalloc(&d_seq, flat.size())); HIP_OK(hipMalloc(&d_pac, l_pac / 4 + 16));
	HIP_OK(hipMalloc(&d_off, (size_t)(n_reads + 1) * 8)); HIP_OK(hipMalloc(&d_len, (size_t)n_reads * 4));
	HIP_OK(hipMalloc(&d_req, (size_t)n_req * sizeof(MswReq))); HIP_OK(hipMalloc(&d_res, (size_t)n_req * sizeof(MswRes)));
	HIP_OK(hipMalloc(&d_rows, (size_t)n_req * max_t * 2));
	HIP_OK(hipMemcpy(d_seq, flat.data(), flat.size(), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_pac, pac, l_pac / 4 + 1, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_off, slot.data(), (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_len, lens.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_req, rq.data(), (size_t)n_req * sizeof(MswReq), hipMemcpyHostToDevice));
	Timer tm;
	tm.start(st);
	std::vector<int> h_list(2 * (size_t)n_req + 16);
	int *d_list, *d_tail;
	HIP_OK(hipMalloc(&d_list, (2 * (size_t)n_req + 16) * sizeof(int)));
	HIP_OK(hipMalloc(&d_tail, msw_tail_ints(n_req) * sizeof(int)));
	launch_msw(st, msw_params(opt, l_pac), n_req, d_req, d_seq, d_off, d_len, d_pac, d_res, d_rows, max_len, rq.data(), lens.data(), h_list.data(), d_list,
	           d_tail);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	static_assert(sizeof(MswRes) == 32, "MswRes layout");
	HIP_OK(hipMemcpy(out8, d_res, (size_t)n_req * sizeof(MswRes), hipMemcpyDeviceToHost));
	(void)hipFree(d_seq); (void)hipFree(d_pac); (void)hipFree(d_off); (void)hipFree(d_len); (void)hipFree(d_req); (void)hipFree(d_res);
	(void)hipFree(d_rows); (void)hipFree(d_list); (void)hipFree(d_tail);
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}

// Stage-level entry point of the chaining stage (tests): seeds of n_reads reads -> filtered chains, computed by
// chain_kernel (which = 0) or by the host path (which = 1).  Per read r the output is a run of int64 starting at
// out[out_off[r]]: n_chains (-1 = the device declines the read), then per chain
//   rid, n_seeds, far_beg, far_end, rmax0, rmax1, frac_rep (float bits), and n_seeds x (rbeg, qbeg, len) in visiting order.
// out must hold 1 + 7 * 9... entries per read in the worst case; the caller sizes it as n_reads + 8 * total_seeds + ...
extern "C" int64_t mi355x_chain_batch(const mem_opt_t *opt, const bntseq_t *bns, int n_reads, const int *lens, const int *l_rep,
                                      const int64_t *seed_off, const uint64_t *rbeg, const int32_t *qbeg_len, int which, int64_t *out,
                                      int64_t out_cap, int64_t *out_off)
{
	using namespace mbw;
	const int64_t S = seed_off[n_reads];
	int max_len = 0;
	for (int i = 0; i < n_reads; ++i) max_len = std::max(max_len, lens[i]);
	const int TS = max_len + 2;
	std::vector<int> tab;
	c2a_length_tables(opt, max_len, tab);
	std::vector<int> nseeds(n_reads);
	for (int i = 0; i < n_reads; ++i) nseeds[i] = (int)(seed_off[i + 1] - seed_off[i]);
	std::vector<int> nch(n_reads, 0);
	std::vector<DevChain> chains(std::max<int64_t>(S, 1));
	std::vector<DevSeed> seeds(std::max<int64_t>(S, 1));
	if (which == 0) {
		int nd = 0;
		if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
		std::vector<int64_t> ann_off;
		std::vector<uint8_t> ann_alt;
		contig_table(bns, ann_off, ann_alt);
		int *d_len, *d_ns, *d_lrep, *d_tab, *d_nch; int64_t *d_so, *d_ao; uint64_t *d_sa; int32_t *d_qbl; uint8_t *d_aa;
		DevChain *d_ch; DevSeed *d_sd; unsigned int *d_srt;
		HIP_OK(hipMalloc(&d_len, n_reads * 4 + 4)); HIP_OK(hipMalloc(&d_ns, n_reads * 4 + 4)); HIP_OK(hipMalloc(&d_lrep, n_reads * 4 + 4));
		HIP_OK(hipMalloc(&d_tab, tab.size() * 4)); HIP_OK(hipMalloc(&d_nch, n_reads * 4 + 4)); HIP_OK(hipMalloc(&d_so, (n_reads + 1) * 8));
		HIP_OK(hipMalloc(&d_ao, ann_off.size() * 8)); HIP_OK(hipMalloc(&d_aa, ann_alt.size())); HIP_OK(hipMalloc(&d_sa, S * 8 + 8));
		HIP_OK(hipMalloc(&d_qbl, S * 8 + 8)); HIP_OK(hipMalloc(&d_ch, (S + 1) * sizeof(DevChain))); HIP_OK(hipMalloc(&d_sd, (S + 1) * sizeof(DevSeed)));
		HIP_OK(hipMalloc(&d_srt, (S + 1) * 4));
		HIP_OK(hipMemcpy(d_len, lens, n_reads * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_ns, nseeds.data(), n_reads * 4, hipMemcpyHostToDevice));
		HIP_OK(hipMemcpy(d_lrep, l_rep, n_reads * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
		HIP_OK(hipMemcpy(d_so, seed_off, (n_reads + 1) * 8, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_ao, ann_off.data(), ann_off.size() * 8, hipMemcpyHostToDevice));
		HIP_OK(hipMemcpy(d_aa, ann_alt.data(), ann_alt.size(), hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_sa, rbeg, S * 8, hipMemcpyHostToDevice));
		HIP_OK(hipMemcpy(d_qbl, qbeg_len, S * 8, hipMemcpyHostToDevice));
		void *d_scr = nullptr;
		HIP_OK(hipMalloc(&d_scr, chain_scratch_bytes(n_reads)));
		launch_chain(0, chain_params(opt, bns->l_pac), n_reads, d_len, d_ns, d_lrep, d_so, d_sa, d_qbl, d_ao, d_aa, bns->n_seqs, d_tab, TS, d_ch, d_sd, d_srt, d_nch, d_scr);
		HIP_OK(hipDeviceSynchronize());
		(void)hipFree(d_scr);
		HIP_OK(hipMemcpy(nch.data(), d_nch, n_reads * 4, hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy((void *)chains.data(), d_ch, S * sizeof(DevChain), hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy((void *)seeds.data(), d_sd, S * sizeof(DevSeed), hipMemcpyDeviceToHost));
		(void)hipFree(d_len); (void)hipFree(d_ns); (void)hipFree(d_lrep); (void)hipFree(d_tab); (void)hipFree(d_nch); (void)hipFree(d_so); (void)hipFree(d_ao);
		(void)hipFree(d_aa); (void)hipFree(d_sa); (void)hipFree(d_qbl); (void)hipFree(d_ch); (void)hipFree(d_sd); (void)hipFree(d_srt);
	} else {
		ChainScratch scr;
		std::vector<HSeed> hs;
		std::vector<HChain *> ch;
		std::vector<uint64_t> key;
		for (int i = 0; i < n_reads; ++i) {
			const int ns = nseeds[i];
			if (ns == 0) continue;
			hs.resize(ns);
			for (int k = 0; k < ns; ++k) {
				const int64_t so = seed_off[i] + k;
				hs[k].rbeg = (int64_t)rbeg[so]; hs[k].qbeg = qbeg_len[2 * so]; hs[k].len = hs[k].score = qbeg_len[2 * so + 1];
			}
			chains_from_seeds(opt, bns, lens[i], hs.data(), ns, l_rep[i], scr, ch);
			chain_filter(opt, scr, ch);
			int64_t cur = seed_off[i];
			int c = 0;
			for (const HChain *cp : ch) {
				DevChain &d = chains[seed_off[i] + c];
				pack_chain_for_device(bns, *cp, lens[i], tab.data(), key, d, seeds.data() + cur);
				d.seed_beg = (int)cur;
				cur += d.n_seeds;
				++c;
			}
			nch[i] = c;
		}
	}
	int64_t at = 0;
	for (int i = 0; i < n_reads; ++i) {
		out_off[i] = at;
		if (at + 1 > out_cap) return -1;
		out[at++] = nch[i];
		for (int c = 0; c < nch[i]; ++c) {
			const DevChain &d = chains[seed_off[i] + c];
			if (at + 7 + 3 * (int64_t)d.n_seeds > out_cap) return -1;
			uint32_t fb;
			memcpy(&fb, &d.frac_rep, 4);
			out[at++] = d.rid; out[at++] = d.n_seeds; out[at++] = d.far_beg; out[at++] = d.far_end; out[at++] = d.rmax0; out[at++] = d.rmax1; out[at++] = fb;
			for (int k = 0; k < d.n_seeds; ++k) {
				const DevSeed &s = seeds[d.seed_beg + k];
				out[at++] = s.rbeg; out[at++] = s.qbeg; out[at++] = s.len;
			}
		}
	}
	out_off[n_reads] = at;
	return at;
}

// Stage-level entry point of chain -> regions (tests): see include/mpibwa_amd.h.  The chains are packed by the library's own
// pack_chain_for_device and laid out as the pipeline lays out device-chained reads (layout 0: read r owns the slots from seed_off[r],
// which leaves room behind its seeds as the seeding counts do) or host-chained ones (layout 1: dense, behind S slots); then the
// pipeline's sequence: the length tables, the launch order, the chain groups with their round trip, c2a_kernel, reg_pack_kernel.
extern "C" int64_t mi355x_c2a_batch(const mem_opt_t *opt, const bntseq_t *bns, int n_reads, const uint8_t *reads, const int64_t *off,
                                    const int *n_chains, const int *chain_rid, const float *chain_frac, const int *chain_nseeds,
                                    const int64_t *seed_rbeg, const int *seed_qbeg, const int *seed_len, const int *seed_score,
                                    int heavy_t, int early, int layout, int64_t *out, int64_t out_cap, int64_t *out_off,
                                    uint64_t *stat4, int *n_units)
{
	using namespace mbw;
	need_index();
	if (bns->l_pac != g_idx.l_pac) die("mi355x_c2a_batch: the index given is not the resident one");
	if (layout != 0 && layout != 1) die("mi355x_c2a_batch: layout %d", layout);
	if (n_reads <= 0) return 0;
	const int64_t l_pac = bns->l_pac;
	int max_len = 0;
	std::vector<int> lens(n_reads);
	for (int i = 0; i < n_reads; ++i) { lens[i] = (int)(off[i + 1] - off[i]); max_len = std::max(max_len, lens[i]); }
	std::vector<int> tab;
	c2a_length_tables(opt, max_len, tab);
	const int TS = max_len + 2;
	// the chains through the library's packing; every seed checked against what mem_chain guarantees, so that no window leaves the index
	std::vector<int> cbeg(n_reads + 1, 0), sbeg(n_reads + 1, 0), nseeds(n_reads, 0);
	int64_t NC = 0, NS = 0;
	for (int i = 0; i < n_reads; ++i) {
		cbeg[i] = (int)NC; sbeg[i] = (int)NS;
		for (int c = 0; c < n_chains[i]; ++c) nseeds[i] += chain_nseeds[NC + c];
		NC += n_chains[i]; NS += nseeds[i];
	}
	cbeg[n_reads] = (int)NC; sbeg[n_reads] = (int)NS;
	std::vector<DevChain> pch(std::max<int64_t>(NC, 1));
	std::vector<DevSeed> psd(std::max<int64_t>(NS, 1));
	{
		HChain ch;
		std::vector<uint64_t> key;
		int64_t s = 0;
		for (int i = 0; i < n_reads; ++i)
			for (int c = cbeg[i]; c < cbeg[i + 1]; ++c) {
				ch.rid = chain_rid[c]; ch.frac_rep = chain_frac[c];
				ch.seeds.resize(chain_nseeds[c]);
				if (ch.rid < 0 || ch.rid >= bns->n_seqs) die("mi355x_c2a_batch: chain %d: rid %d", c, ch.rid);
				for (int k = 0; k < chain_nseeds[c]; ++k, ++s) {
					HSeed &h = ch.seeds[k];
					h.rbeg = seed_rbeg[s]; h.qbeg = seed_qbeg[s]; h.len = seed_len[s]; h.score = seed_score[s];
					if (h.len <= 0 || h.qbeg < 0 || h.qbeg + h.len > lens[i] || h.rbeg < 0 || h.rbeg + h.len > 2 * l_pac)
						die("mi355x_c2a_batch: read %d, chain %d: seed %d out of bounds", i, c, k);
				}
				DevChain &d = pch[c];
				pack_chain_for_device(bns, ch, lens[i], tab.data(), key, d, psd.data() + (s - chain_nseeds[c]));
				for (int k = 0; k < chain_nseeds[c]; ++k) {
					const DevSeed &t = psd[s - chain_nseeds[c] + k];
					if (t.rbeg < d.rmax0 || t.rbeg + t.len > d.rmax1) die("mi355x_c2a_batch: read %d, chain %d: a seed leaves the chain's contig or strand", i, c);
				}
			}
	}
	// slots: layout 0 gives read i the run seed_off[i] .. (its seeds, and a few more: the seeding stage counts the seeds before chaining)
	// for chains, seeds and regions alike; layout 1 puts them densely behind a base, the chains and the seeds each from their own offset
	std::vector<int> chain_beg(n_reads), chain_cnt(n_reads), reg_beg(n_reads);
	std::vector<int64_t> seed_at(n_reads);
	int64_t n_slots = 0, n_chain_slots = 0;
	if (layout == 0) {
		int64_t so = 0;
		for (int i = 0; i < n_reads; ++i) {
			chain_beg[i] = reg_beg[i] = (int)so; seed_at[i] = so;
			so += std::max(nseeds[i], n_chains[i]) + (i % 3);
		}
		n_slots = n_chain_slots = so;
	} else {
		const int64_t base = NS + 5;
		for (int i = 0; i < n_reads; ++i) { chain_beg[i] = (int)(base + cbeg[i]); reg_beg[i] = (int)(base + sbeg[i]); seed_at[i] = base + sbeg[i]; }
		n_slots = base + NS; n_chain_slots = base + NC;
	}
	if (n_slots > 0x7fffffff) die("mi355x_c2a_batch: too many seeds");
	std::vector<DevChain> hch(std::max<int64_t>(n_chain_slots, 1));
	std::vector<DevSeed> hsd(std::max<int64_t>(n_slots, 1));
	std::vector<unsigned int> hsrt(std::max<int64_t>(n_slots, 1), 0);
	for (int i = 0; i < n_reads; ++i) {
		chain_cnt[i] = n_chains[i];
		int64_t at = seed_at[i];
		for (int c = 0; c < n_chains[i]; ++c) {
			DevChain d = pch[cbeg[i] + c];
			const int64_t from = sbeg[i] + (at - seed_at[i]);
			for (int k = 0; k < d.n_seeds; ++k) { hsd[at + k] = psd[from + k]; hsrt[at + k] = (unsigned int)k; }
			d.seed_beg = (int)at;
			at += d.n_seeds;
			hch[chain_beg[i] + c] = d;
		}
	}
	// the reads in 16-byte slots, 16 bytes of padding behind the last one (the kernel stages a read 4 bytes at a time)
	std::vector<int64_t> slot(n_reads + 1, 0);
	for (int i = 0; i < n_reads; ++i) slot[i + 1] = slot[i] + ((lens[i] + 15) & ~15);
	std::vector<uint8_t> flat(slot[n_reads] + 16, 4);
	for (int i = 0; i < n_reads; ++i) memcpy(flat.data() + slot[i], reads + off[i], (size_t)lens[i]);
	std::vector<int> order(n_reads);
	c2a_launch_order(n_reads, nseeds.data(), order.data());

	hipStream_t st = 0;
	uint8_t *d_seq; int64_t *d_off; int *d_len, *d_cbeg, *d_ccnt, *d_rbeg, *d_nregs, *d_tab, *d_order, *d_reg_pos;
	DevChain *d_ch; DevSeed *d_sd; unsigned int *d_srt; DevReg *d_regs, *d_packed; unsigned long long *d_stat;
	HIP_OK(hipMalloc(&d_seq, flat.size())); HIP_OK(hipMalloc(&d_off, (size_t)(n_reads + 1) * 8)); HIP_OK(hipMalloc(&d_len, (size_t)n_reads * 4));
	HIP_OK(hipMalloc(&d_cbeg, (size_t)n_reads * 4)); HIP_OK(hipMalloc(&d_ccnt, (size_t)n_reads * 4)); HIP_OK(hipMalloc(&d_rbeg, (size_t)n_reads * 4));
	HIP_OK(hipMalloc(&d_nregs, (size_t)(n_reads + 1) * 4)); HIP_OK(hipMalloc(&d_tab, tab.size() * 4)); HIP_OK(hipMalloc(&d_order, (size_t)n_reads * 4));
	HIP_OK(hipMalloc(&d_reg_pos, (size_t)(n_reads + 1) * 4));
	HIP_OK(hipMalloc(&d_ch, hch.size() * sizeof(DevChain))); HIP_OK(hipMalloc(&d_sd, hsd.size() * sizeof(DevSeed)));
	HIP_OK(hipMalloc(&d_srt, hsrt.size() * 4)); HIP_OK(hipMalloc(&d_regs, hsd.size() * sizeof(DevReg)));
	HIP_OK(hipMalloc(&d_packed, hsd.size() * sizeof(DevReg))); HIP_OK(hipMalloc(&d_stat, C2A_STAT_SLOTS * 64));
	const size_t tmp_bytes = reg_pack_tmp_bytes(n_reads);
	void *d_tmp;
	HIP_OK(hipMalloc(&d_tmp, tmp_bytes));
	HIP_OK(hipMemcpy(d_seq, flat.data(), flat.size(), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_off, slot.data(), (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_len, lens.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_cbeg, chain_beg.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_ccnt, chain_cnt.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_rbeg, reg_beg.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_order, order.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_ch, hch.data(), hch.size() * sizeof(DevChain), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_sd, hsd.data(), hsd.size() * sizeof(DevSeed), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_srt, hsrt.data(), hsrt.size() * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemset(d_stat, 0, C2A_STAT_SLOTS * 64));
	{
		C2aGroupBufs B;
		const C2aUnits units = c2a_prepare_units(st, B, heavy_t, n_reads, chain_cnt.data(), (size_t)std::max<int64_t>(n_chain_slots, 1), d_cbeg, d_rbeg,
		                                         d_ch, d_nregs);
		C2aParams cp;
		ExtParams ep;
		c2a_params(opt, l_pac, early, cp, ep);
		launch_c2a(st, cp, ep, n_reads, d_seq, d_off, d_len, d_cbeg, d_ccnt, d_ch, d_sd, d_srt, d_rbeg, d_regs, d_nregs, d_tab, TS,
		           (const uint8_t *)g_idx.d_pac, d_stat, max_len, d_order, units.max_units > 0 ? &units : nullptr);
		launch_reg_pack(st, n_reads, d_rbeg, d_nregs, d_reg_pos, d_regs, d_packed, d_tmp, tmp_bytes, units.max_units > 0 ? &units : nullptr, d_cbeg, d_ccnt);
		HIP_OK(hipStreamSynchronize(st));
		HIP_OK(hipGetLastError());
		if (n_units) *n_units = units.max_units;
		B.heavy.release(); B.hoff.release(); B.scratch.release(); B.clist.release(); B.ustart.release(); B.unit_rd.release();
		B.unit_av.release(); B.nunits.release(); B.c_rabs.release(); B.c_rcnt.release();
		if (B.h_heavy.p) HIP_OK(hipHostFree(B.h_heavy.p));
		if (B.h_hoff.p) HIP_OK(hipHostFree(B.h_hoff.p));
		if (B.h_nunits.p) HIP_OK(hipHostFree(B.h_nunits.p));
	}
	std::vector<int> nregs(n_reads), reg_pos(n_reads + 1);
	std::vector<unsigned long long> stat(C2A_STAT_SLOTS * 8);
	HIP_OK(hipMemcpy(nregs.data(), d_nregs, (size_t)n_reads * 4, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(reg_pos.data(), d_reg_pos, (size_t)(n_reads + 1) * 4, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(stat.data(), d_stat, C2A_STAT_SLOTS * 64, hipMemcpyDeviceToHost));
	std::vector<DevReg> regs(std::max(reg_pos[n_reads], 1));
	HIP_OK(hipMemcpy((void *)regs.data(), d_packed, (size_t)reg_pos[n_reads] * sizeof(DevReg), hipMemcpyDeviceToHost));
	(void)hipFree(d_seq); (void)hipFree(d_off); (void)hipFree(d_len); (void)hipFree(d_cbeg); (void)hipFree(d_ccnt); (void)hipFree(d_rbeg);
	(void)hipFree(d_nregs); (void)hipFree(d_tab); (void)hipFree(d_order); (void)hipFree(d_reg_pos); (void)hipFree(d_ch); (void)hipFree(d_sd);
	(void)hipFree(d_srt); (void)hipFree(d_regs); (void)hipFree(d_packed); (void)hipFree(d_stat); (void)hipFree(d_tmp);
	for (int k = 0; k < 4; ++k) {
		uint64_t t = 0;
		for (int sl = 0; sl < C2A_STAT_SLOTS; ++sl) t += stat[(size_t)sl * 8 + k];
		if (stat4) stat4[k] = t;
	}
	int64_t at = 0;
	for (int i = 0; i < n_reads; ++i) {
		out_off[i] = at;
		if (at + 1 + 11 * (int64_t)nregs[i] > out_cap) return -1;
		out[at++] = nregs[i];
		for (int k = 0; k < nregs[i]; ++k) {
			const DevReg &a = regs[reg_pos[i] + k];
			uint32_t fb;
			memcpy(&fb, &a.frac_rep, 4);
			const int64_t v[11] = {a.rb, a.re, a.qb, a.qe, a.rid, a.score, a.truesc, a.w, a.seedcov, a.seedlen0, (int64_t)fb};
			for (int f = 0; f < 11; ++f) out[at++] = v[f];
		}
	}
	out_off[n_reads] = at;
	return at;
}

// Stage-level entry point of the CIGAR / MD / NM kernel (tests): n_req regions of reads of a batch against windows of the
// packed reference `pac`, through mem_reg2aln's band-doubling loop (src/bwamem.c:1106-1122) exactly as the SAM stage asks
// for them.  which = 0: the product's dispatch (no-DP / narrow band / full size); 1: DP requests straight to the full-size
// instantiation.  out_hdr5 per request: score, NM, n_cigar, md_len, flags.
extern "C" int mi355x_global_batch(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, int n_reads, const uint8_t *reads,
                                   const int64_t *off, int n_req, const int64_t *rb, const int64_t *re, const int *read,
                                   const int *qb, const int *qe, const int *w, const int *truesc, int which,
                                   int *out_hdr5, uint32_t *cigar_out, int cigar_cap, char *md_out, int md_cap, double *kernel_ms)
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n_req <= 0) return 0;
	hipStream_t st = 0;
	std::vector<int64_t> slot(n_reads + 1);
	int max_len = 0;
	slot[0] = 0;
	for (int i = 0; i < n_reads; ++i) {
		const int len = (int)(off[i + 1] - off[i]);
		slot[i + 1] = slot[i] + ((len + 15) & ~15);
		max_len = std::max(max_len, len);
	}
	std::vector<uint8_t> flat(slot[n_reads] + 16, 4);
	for (int i = 0; i < n_reads; ++i) memcpy(flat.data() + slot[i], reads + off[i], (size_t)(off[i + 1] - off[i]));
	std::vector<AlnReq> rq(n_req);
	for (int i = 0; i < n_req; ++i) {
		if (read[i] < 0 || read[i] >= n_reads || rb[i] < 0 || re[i] > 2 * l_pac) die("mi355x_global_batch: bad request %d", i);
		rq[i].rb = rb[i]; rq[i].re = re[i]; rq[i].read = read[i]; rq[i].qb = qb[i]; rq[i].qe = qe[i]; rq[i].w2 = w[i]; rq[i].truesc = truesc[i];
		rq[i].pad = 0;
	}
	std::vector<int> gaptab;
	cigar_gap_table(opt, max_len, gaptab);
	// (not aln_pool_bytes: a test may ask for nothing but long gapped alignments, whose CIGAR and MD outgrow the pipeline's 96-byte average)
	const size_t pool_bytes = (size_t)n_req * (4 * 96 + 768) + ((size_t)48 << 20);
	uint8_t *d_seq, *d_pac, *d_pool; int64_t *d_off; AlnReq *d_req; AlnHdr *d_hdr; int *d_gap, *d_lists; unsigned long long *d_cnt;
	HIP_OK(hipMalloc(&d_seq, flat.size())); HIP_OK(hipMalloc(&d_pac, l_pac / 4 + 16)); HIP_OK(hipMalloc(&d_pool, pool_bytes));
	HIP_OK(hipMalloc(&d_off, (size_t)(n_reads + 1) * 8)); HIP_OK(hipMalloc(&d_req, (size_t)n_req * sizeof(AlnReq)));
	HIP_OK(hipMalloc(&d_hdr, (size_t)n_req * sizeof(AlnHdr))); HIP_OK(hipMalloc(&d_gap, gaptab.size() * 4));
	HIP_OK(hipMalloc(&d_lists, (size_t)n_req * 3 * 4)); HIP_OK(hipMalloc(&d_cnt, 256));
	HIP_OK(hipMemcpy(d_seq, flat.data(), flat.size(), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_pac, pac, l_pac / 4 + 1, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_off, slot.data(), (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_req, rq.data(), (size_t)n_req * sizeof(AlnReq), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_gap, gaptab.data(), gaptab.size() * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemset(d_cnt, 0, 256));
	AlnParams ap;
	ExtParams ep;
	aln_params(opt, l_pac, ap, ep);
	Timer tm;
	tm.start(st);
	launch_aln(st, ap, ep, n_req, d_req, d_seq, d_off, d_pac, d_gap, d_hdr, d_pool, d_cnt, pool_bytes, max_len, max_len + 256, d_lists, which != 0);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	std::vector<AlnHdr> hdr(n_req);
	std::vector<uint8_t> pool(pool_bytes);
	HIP_OK(hipMemcpy((void *)hdr.data(), d_hdr, (size_t)n_req * sizeof(AlnHdr), hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(pool.data(), d_pool, pool_bytes, hipMemcpyDeviceToHost));
	(void)hipFree(d_seq); (void)hipFree(d_pac); (void)hipFree(d_pool); (void)hipFree(d_off); (void)hipFree(d_req); (void)hipFree(d_hdr);
	(void)hipFree(d_gap); (void)hipFree(d_lists); (void)hipFree(d_cnt);
	int rc = 0;
	for (int i = 0; i < n_req; ++i) {
		const AlnHdr &h = hdr[i];
		int *o = out_hdr5 + 5 * (size_t)i;
		o[0] = h.score; o[1] = h.NM; o[2] = h.n_cigar; o[3] = h.md_len; o[4] = h.flags;
		if (h.flags) continue;
		if (h.n_cigar > cigar_cap || h.md_len > md_cap) { rc = -1; continue; }
		memcpy(cigar_out + (size_t)cigar_cap * i, pool.data() + (size_t)h.pool_off * 4, (size_t)h.n_cigar * 4);
		memcpy(md_out + (size_t)md_cap * i, pool.data() + (size_t)h.pool_off * 4 + (size_t)h.n_cigar * 4, (size_t)h.md_len);
	}
	if (kernel_ms) *kernel_ms = ms;
	return rc;
}

// Stage-level entry point of the SAM text kernel (tests): the CIGAR kernel and sam_emit_kernel on chosen line descriptors, queued on one
// stream through the pipeline's own queue_aln_sam().  Reads as nt4 codes in 16-byte
// slots like the pipeline's, qualities (or none) at the same places, names back to back; the read group is bwa_rg_id.  The arena is
// followed by SAM_GUARD bytes that no record may touch; arena and guard are filled with SAM_GUARD_BYTE before the launch.
#define SAM_GUARD 4096
#define SAM_GUARD_BYTE 0xA5
extern "C" size_t mi355x_sam_arena_bytes(int n_reads, int max_len) { return sam_arena_bytes(n_reads, max_len); }
// (ends = 2: a unit of req_base is a pair, the paired instantiation of the kernel; ends = 1: a unit is a read, the single-end one)
static int sam_batch(const char *who, int ends, const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_units, const uint8_t *reads,
                     const int64_t *off, const uint8_t *quals, const char *names, const int *name_off, const void *desc_, const void *reqs_,
                     const int *req_base, size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off, uint8_t *arena_out,
                     unsigned long long *cursor, void *hdr_out)
{
	using namespace mbw;
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n_units <= 0) return 0;
	hipStream_t st = 0;
	const int n = ends * n_units, n_req = req_base[n_units];
	const int64_t l_pac = bns->l_pac;
	const SamDesc *desc = (const SamDesc *)desc_;
	const AlnReq *reqs = (const AlnReq *)reqs_;
	std::vector<int64_t> slot(n + 1);
	std::vector<int> lens(n);
	int max_len = 0;
	slot[0] = 0;
	for (int i = 0; i < n; ++i) {
		lens[i] = (int)(off[i + 1] - off[i]);
		if (lens[i] <= 0 || name_off[i + 1] < name_off[i]) die("%s: bad read %d", who, i);
		slot[i + 1] = slot[i] + ((lens[i] + 15) & ~15);
		max_len = std::max(max_len, lens[i]);
	}
	// nothing the kernels index with may point outside what was uploaded
	if (req_base[0] != 0 || n_req < 0) die("%s: bad req_base", who);
	for (int k = 0; k < n_units; ++k) {
		if (req_base[k + 1] < req_base[k]) die("%s: bad req_base at unit %d", who, k);
		if (ends == 2 && (desc[2 * k].req >= 0) != (desc[2 * k + 1].req >= 0)) die("%s: pair %d has one record of the device's only", who, k);
		for (int e = 0; e < ends; ++e) {
			const int r = ends * k + e;
			const SamDesc &d = desc[r];
			if (d.req < 0) continue;
			const int q = req_base[k] + d.req;
			if (q >= req_base[k + 1] || d.rid < 0 || d.rid >= bns->n_seqs || reqs[q].read != r) die("%s: bad descriptor %d", who, r);
			if (d.rb < 0 || d.re > 2 * l_pac || d.rb >= d.re || d.qb < 0 || d.qe > lens[r] || d.qb > d.qe) die("%s: bad region %d", who, r);
			for (int j = 1; j <= (d.flag >> SAM_XA_SHIFT & SAM_XA_MASK); ++j)   // its XA entries' requests follow its own
				if (q + j >= req_base[k + 1] || reqs[q + j].read != r || reqs[q + j].pad < 0 || reqs[q + j].pad >= bns->n_seqs || reqs[q + j].rb >= reqs[q + j].re)
					die("%s: bad XA request %d of descriptor %d", who, j, r);
		}
	}
	for (int q = 0; q < n_req; ++q) {
		const AlnReq &r = reqs[q];
		if (r.read < 0) continue;
		if (r.read >= n || r.rb < 0 || r.re > 2 * l_pac || r.rb > r.re || r.qb < 0 || r.qb > r.qe || r.qe > lens[r.read]) die("%s: bad request %d", who, q);
	}
	std::vector<uint8_t> flat(slot[n] + 16, 4), fq;
	for (int i = 0; i < n; ++i) memcpy(flat.data() + slot[i], reads + off[i], (size_t)lens[i]);
	if (quals) {
		fq.assign(flat.size(), 0);
		for (int i = 0; i < n; ++i) memcpy(fq.data() + slot[i], quals + off[i], (size_t)lens[i]);
	}
	std::vector<int> gaptab;
	cigar_gap_table(opt, max_len, gaptab);
	std::vector<int64_t> ann_off;
	std::vector<uint8_t> ann_alt;
	contig_table(bns, ann_off, ann_alt);
	std::vector<int> cno;
	std::vector<char> cn;
	contig_names(bns, cn, cno);
	const SamParams sp = sam_params(l_pac, quals != nullptr);
	if (!arena_bytes) arena_bytes = sam_arena_bytes(n, max_len);
	const size_t pool_bytes = aln_pool_bytes((size_t)std::max(n_req, 1));
	const size_t n_names = (size_t)name_off[n];
	uint8_t *d_seq, *d_qual = nullptr, *d_pac, *d_pool, *d_names, *d_arena; char *d_cn; int64_t *d_off, *d_ao; AlnReq *d_req; AlnHdr *d_hdr;
	int *d_gap, *d_lists, *d_len, *d_noff, *d_cno, *d_base, *d_olen; unsigned long long *d_cnt, *d_used, *d_ooff; SamDesc *d_desc;
	HIP_OK(hipMalloc(&d_seq, flat.size())); HIP_OK(hipMalloc(&d_pac, l_pac / 4 + 16)); HIP_OK(hipMalloc(&d_pool, pool_bytes));
	if (quals) HIP_OK(hipMalloc(&d_qual, fq.size()));
	HIP_OK(hipMalloc(&d_off, (size_t)(n + 1) * 8)); HIP_OK(hipMalloc(&d_len, (size_t)n * 4)); HIP_OK(hipMalloc(&d_req, (size_t)std::max(n_req, 1) * sizeof(AlnReq)));
	HIP_OK(hipMalloc(&d_hdr, (size_t)std::max(n_req, 1) * sizeof(AlnHdr))); HIP_OK(hipMalloc(&d_gap, gaptab.size() * 4));
	HIP_OK(hipMalloc(&d_lists, (size_t)std::max(n_req, 1) * 3 * 4)); HIP_OK(hipMalloc(&d_cnt, 256)); HIP_OK(hipMalloc(&d_used, 64));
	HIP_OK(hipMalloc(&d_names, n_names + 64)); HIP_OK(hipMalloc(&d_noff, (size_t)(n + 1) * 4)); HIP_OK(hipMalloc(&d_cn, cn.size() + 64));
	HIP_OK(hipMalloc(&d_cno, cno.size() * 4)); HIP_OK(hipMalloc(&d_ao, ann_off.size() * 8)); HIP_OK(hipMalloc(&d_base, (size_t)(n_units + 1) * 4));
	HIP_OK(hipMalloc(&d_desc, (size_t)n * sizeof(SamDesc))); HIP_OK(hipMalloc(&d_arena, arena_bytes + SAM_GUARD));
	HIP_OK(hipMalloc(&d_ooff, (size_t)n * 8)); HIP_OK(hipMalloc(&d_olen, (size_t)n * 4));
	HIP_OK(hipMemcpy(d_seq, flat.data(), flat.size(), hipMemcpyHostToDevice));
	if (quals) HIP_OK(hipMemcpy(d_qual, fq.data(), fq.size(), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_pac, pac, l_pac / 4 + 1, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_off, slot.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_len, lens.data(), (size_t)n * 4, hipMemcpyHostToDevice));
	if (n_req) HIP_OK(hipMemcpy(d_req, reqs, (size_t)n_req * sizeof(AlnReq), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_gap, gaptab.data(), gaptab.size() * 4, hipMemcpyHostToDevice));
	if (n_names) HIP_OK(hipMemcpy(d_names, names, n_names, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_noff, name_off, (size_t)(n + 1) * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_cn, cn.data(), cn.size(), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_cno, cno.data(), cno.size() * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_ao, ann_off.data(), ann_off.size() * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_desc, desc, (size_t)n * sizeof(SamDesc), hipMemcpyHostToDevice));
	HIP_OK(hipMemset(d_hdr, 0, (size_t)std::max(n_req, 1) * sizeof(AlnHdr)));
	HIP_OK(hipMemset(d_arena, SAM_GUARD_BYTE, arena_bytes + SAM_GUARD));
	HIP_OK(hipMemset(d_ooff, 0, (size_t)n * 8));
	HIP_OK(hipMemset(d_olen, 0xff, (size_t)n * 4));
	ChunkDev D;
	D.d_seq = d_seq; D.d_off = d_off; D.d_len = d_len; D.max_len = max_len; D.d_pac = d_pac; D.d_gap = d_gap;
	D.d_qual = d_qual; D.d_names = d_names; D.d_noff = d_noff; D.d_ann_off = d_ao; D.d_ann_names = d_cn; D.d_ann_noff = d_cno;
	AlnSamJob J;
	J.n_req = n_req; J.d_req = d_req; J.d_hdr = d_hdr; J.d_pool = d_pool; J.pool_bytes = pool_bytes; J.d_cnt = d_cnt; J.d_lists = d_lists;
	J.ends = ends; J.n_reads = n; J.d_desc = d_desc; J.h_base = req_base; J.d_base = d_base;
	J.d_arena = d_arena; J.arena_bytes = arena_bytes; J.d_used = d_used; J.d_ooff = d_ooff; J.d_olen = d_olen; J.grid_blocks = grid_blocks;
	queue_aln_sam(st, opt, l_pac, D, sp, J);
	HIP_OK(hipStreamSynchronize(st));
	HIP_OK(hipGetLastError());
	HIP_OK(hipMemcpy(out_len, d_olen, (size_t)n * 4, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(out_off, d_ooff, (size_t)n * 8, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(arena_out, d_arena, arena_bytes + SAM_GUARD, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(cursor, d_used, 8, hipMemcpyDeviceToHost));
	if (n_req) HIP_OK(hipMemcpy(hdr_out, d_hdr, (size_t)n_req * sizeof(AlnHdr), hipMemcpyDeviceToHost));
	(void)hipFree(d_seq); (void)hipFree(d_qual); (void)hipFree(d_pac); (void)hipFree(d_pool); (void)hipFree(d_off); (void)hipFree(d_len); (void)hipFree(d_req);
	(void)hipFree(d_hdr); (void)hipFree(d_gap); (void)hipFree(d_lists); (void)hipFree(d_cnt); (void)hipFree(d_used); (void)hipFree(d_names); (void)hipFree(d_noff);
	(void)hipFree(d_cn); (void)hipFree(d_cno); (void)hipFree(d_ao); (void)hipFree(d_base); (void)hipFree(d_desc); (void)hipFree(d_arena); (void)hipFree(d_ooff);
	(void)hipFree(d_olen);
	return 0;
}

extern "C" int mi355x_sam_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_pairs, const uint8_t *reads, const int64_t *off,
                                const uint8_t *quals, const char *names, const int *name_off, const void *desc_, const void *reqs_, const int *req_base,
                                size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off, uint8_t *arena_out,
                                unsigned long long *cursor, void *hdr_out)
{
	return sam_batch("mi355x_sam_batch", 2, opt, bns, pac, n_pairs, reads, off, quals, names, name_off, desc_, reqs_, req_base, arena_bytes, grid_blocks,
	                 out_len, out_off, arena_out, cursor, hdr_out);
}
// The twin for single-end descriptors (mi355x_se_batch's): a unit of req_base is a read, the kernel's single-end instantiation runs
extern "C" int mi355x_sam_se_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_reads, const uint8_t *reads, const int64_t *off,
                                   const uint8_t *quals, const char *names, const int *name_off, const void *desc_, const void *reqs_, const int *req_base,
                                   size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off, uint8_t *arena_out,
                                   unsigned long long *cursor, void *hdr_out)
{
	return sam_batch("mi355x_sam_se_batch", 1, opt, bns, pac, n_reads, reads, off, quals, names, name_off, desc_, reqs_, req_base, arena_bytes, grid_blocks,
	                 out_len, out_off, arena_out, cursor, hdr_out);
}

// Stage-level entry point of the seed enumeration between SMEM and SA lookup (tests): seed_prep_kernel, the pipeline's prefix sum over
// the seed counts, seed_enum_kernel, on chosen intervals (read r: n_intv[r] records of (x0, x1, size, info) from intv[r * cap * 4], in any
// order; n_intv[r] > cap: the kernels look at the first cap).  intv comes back sorted by info; rows / qbeg_len: per seed the BWT row
// and (qbeg, len), read r from seed_off[r].  Returns the number of seeds, or -1 - that number when it exceeds seed_cap (then only
// n_seeds, l_rep and seed_off are valid).
extern "C" int64_t mi355x_seed_batch(int n_reads, int cap, int max_occ, uint64_t *intv, const int *n_intv, int *n_seeds, int *l_rep,
                                     int64_t *seed_off, uint64_t *rows, int32_t *qbeg_len, int64_t seed_cap)
{
	using namespace mbw;
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
	if (n_reads <= 0) return 0;
	if (cap <= 0 || max_occ <= 0) die("mi355x_seed_batch: cap and max_occ must be positive");
	hipStream_t st = 0;
	const size_t n_words = (size_t)n_reads * cap * 4;
	uint64_t *d_intv, *d_rows = nullptr; int *d_nintv, *d_ns, *d_lrep; int64_t *d_so; int32_t *d_qbl = nullptr;
	HIP_OK(hipMalloc(&d_intv, n_words * 8)); HIP_OK(hipMalloc(&d_nintv, (size_t)n_reads * 4)); HIP_OK(hipMalloc(&d_ns, (size_t)n_reads * 4));
	HIP_OK(hipMalloc(&d_lrep, (size_t)n_reads * 4)); HIP_OK(hipMalloc(&d_so, (size_t)(n_reads + 1) * 8));
	HIP_OK(hipMemcpy(d_intv, intv, n_words * 8, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(d_nintv, n_intv, (size_t)n_reads * 4, hipMemcpyHostToDevice));
	launch_seed_prep(st, n_reads, cap, d_intv, d_nintv, max_occ, d_ns, d_lrep);
	HIP_OK(hipStreamSynchronize(st));
	HIP_OK(hipGetLastError());
	HIP_OK(hipMemcpy(n_seeds, d_ns, (size_t)n_reads * 4, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(l_rep, d_lrep, (size_t)n_reads * 4, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(intv, d_intv, n_words * 8, hipMemcpyDeviceToHost));
	seed_off[0] = 0;
	for (int i = 0; i < n_reads; ++i) seed_off[i + 1] = seed_off[i] + n_seeds[i];
	const int64_t S = seed_off[n_reads];
	// the device buffers hold what the intervals themselves allow (min(size, max_occ) + 1 rows each), wherever the counts of
	// seed_prep_kernel put a read: counts that are too small show as seeds of one read over those of the next, never as a write outside
	const bool fits = S <= seed_cap;
	int64_t room = S;
	for (int i = 0; i < n_reads; ++i) {
		if (n_seeds[i] < 0) die("mi355x_seed_batch: read %d counts %d seeds", i, n_seeds[i]);
		int64_t most = 0;
		const int m = std::min(n_intv[i], cap);
		for (int k = 0; k < m; ++k) most += (int64_t)std::min<uint64_t>(intv[((size_t)i * cap + k) * 4 + 2], (uint64_t)max_occ) + 1;
		room = std::max(room, seed_off[i] + most);
	}
	if (fits && S > 0) {
		HIP_OK(hipMalloc(&d_rows, (size_t)room * 8)); HIP_OK(hipMalloc(&d_qbl, (size_t)room * 8));
		HIP_OK(hipMemset(d_rows, 0xff, (size_t)room * 8)); HIP_OK(hipMemset(d_qbl, 0xff, (size_t)room * 8));
		HIP_OK(hipMemcpy(d_so, seed_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice));
		launch_seed_enum(st, n_reads, cap, d_intv, d_nintv, max_occ, d_so, d_rows, d_qbl);
		HIP_OK(hipStreamSynchronize(st));
		HIP_OK(hipGetLastError());
		HIP_OK(hipMemcpy(rows, d_rows, (size_t)S * 8, hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy(qbeg_len, d_qbl, (size_t)S * 8, hipMemcpyDeviceToHost));
	}
	(void)hipFree(d_intv); (void)hipFree(d_nintv); (void)hipFree(d_ns); (void)hipFree(d_lrep); (void)hipFree(d_so); (void)hipFree(d_rows); (void)hipFree(d_qbl);
	return fits ? S : -1 - S;
}
