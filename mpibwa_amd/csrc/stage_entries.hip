// stage_entries.hip — the stage-level C entry points (parity tests, micro-benchmarks): one kernel or one stage of the pipeline on inputs
// chosen by the caller, with device arrays that live for the call (hip_util.h: DevArr).  The pipeline itself does not come through here.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hip_util.h"
#include "device.h"
#include "host.h"

using namespace mbw;

static void need_index()
{
	if (!dev_index().ready) die("index not resident on the device: call mi355x_index_upload() first");
}

static void require_any_device()
{
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) die("no HIP device visible (no CPU fallback)");
}

// Reads of a batch as the kernels expect them: read i in a 16-byte aligned slot from slot[i], true length lens[i], the unused bytes of
// the slots and 16 bytes behind the last one (the kernels stage a read several bytes at a time) filled with `pad`
struct PackedReads {
	std::vector<int> lens;
	std::vector<int64_t> slot;
	std::vector<uint8_t> flat;
	int max_len = 0;
};
static PackedReads pack_reads(int n, const uint8_t *reads, const int64_t *off, uint8_t pad)
{
	PackedReads R;
	R.lens.resize(n);
	R.slot.assign(n + 1, 0);
	for (int i = 0; i < n; ++i) {
		R.lens[i] = (int)(off[i + 1] - off[i]);
		R.slot[i + 1] = R.slot[i] + ((R.lens[i] + 15) & ~15);
		R.max_len = std::max(R.max_len, R.lens[i]);
	}
	R.flat.assign(R.slot[n] + 16, pad);
	for (int i = 0; i < n; ++i) memcpy(R.flat.data() + R.slot[i], reads + off[i], (size_t)R.lens[i]);
	return R;
}

// Stage entry of se_simple_kernel (se_kernel.hip) for parity tests: n_reads single-end reads given by their regions as they stand after
// phase 1 (regs: PR_MAXREG DevReg records per read, n_regs per read); status[i] = 1: decided — desc[i] (SamDesc) and req[i] (AlnReq) are
// what mem_reg2sam reports with one line; else the code of the test that sent the read to the host (device.h: SE_HOST_*).
extern "C" int mi355x_se_batch(const mem_opt_t *opt, const bntseq_t *bns, int64_t n_processed, int n_reads, const void *regs, const int *n_regs,
                               int max_len, uint8_t *status, void *desc, void *req)
{
	require_any_device();
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
	DevArr<DevReg> d_first(n * PR_MAXREG * sizeof(DevReg), regs);
	DevArr<int> d_nf(n * 4, n_regs);
	DevArr<uint8_t> d_ok(n, ok.data()), d_aa(ann_alt.size(), ann_alt.data()), d_st(n);
	DevArr<double> d_tab(tab.size() * 8, tab.data());
	DevArr<AlnReq> d_rq(n * sizeof(AlnReq));
	DevArr<SamDesc> d_ds(n * sizeof(SamDesc));
	launch_se_simple(0, pp, n_reads, d_first, d_nf, d_ok, d_aa, d_tab, d_st, d_rq, d_ds);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	d_st.download(status, n);
	d_ds.download(desc, n * sizeof(SamDesc));
	d_rq.download(req, n * sizeof(AlnReq));
	return 0;
}

// Stage entry of the redundancy pass on the device (dedup_kernel.hip) for parity tests: n_reads reads given by their raw region lists as
// mem_chain2aln leaves them (regs: DevReg records back to back, read r owns regs[reg_off[r] .. reg_off[r + 1])), through the pipeline's own
// launch sequence (launch_dedup: the lane-per-read kernel, which lists the longer reads, then the wave kernel).  status[r], m[r] as
// device.h describes them (DD_*); keep (reg_off[n_reads] ints) goes up as the caller filled it and comes back as the device left it.
extern "C" int mi355x_dedup_batch(const mem_opt_t *opt, const bntseq_t *bns, int n_reads, const void *regs, const int *reg_off, uint8_t *status, int *m,
                                  int *keep, double *kernel_ms)
{
	require_any_device();
	if (kernel_ms) *kernel_ms = 0;
	if (n_reads <= 0) return 0;
	const size_t n = (size_t)n_reads;
	if (reg_off[0] != 0) die("mi355x_dedup_batch: reg_off[0] must be 0");
	std::vector<int> nregs(n);
	for (size_t i = 0; i < n; ++i) {
		if (reg_off[i + 1] < reg_off[i]) die("mi355x_dedup_batch: reg_off decreases at read %zu", i);
		nregs[i] = reg_off[i + 1] - reg_off[i];
	}
	const size_t NR = (size_t)reg_off[n];
	hipStream_t st = 0;
	DevArr<DevReg> d_packed(std::max<size_t>(NR, 1) * sizeof(DevReg), regs, NR * sizeof(DevReg));
	DevArr<int> d_pos((n + 1) * 4, reg_off), d_nr(n * 4, nregs.data()), d_m(n * 4), d_keep(std::max<size_t>(NR, 1) * 4, keep, NR * 4);
	DevArr<int> d_list(dedup_list_ints(n_reads) * 4);
	DevArr<uint8_t> d_st(n);
	d_st.zero();
	d_m.fill(0xff);
	Timer tm;
	tm.start(st);
	launch_dedup(st, dedup_params(opt, bns->l_pac), n_reads, d_packed, d_pos, d_nr, d_st, d_m, d_keep, d_list);
	const double ms = tm.stop(st);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	d_st.download(status, n);
	d_m.download(m, n * 4);
	if (NR) d_keep.download(keep, NR * 4);
	if (kernel_ms) *kernel_ms = ms;
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
	require_any_device();
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
	DevArr<DevReg> d_first(n * PR_MAXREG * sizeof(DevReg), regs);
	DevArr<int> d_nf(n * 4, n_regs);
	DevArr<uint8_t> d_ok(n_pairs, ok.data()), d_aa(ann_alt.size(), ann_alt.data()), d_st(n_pairs);
	DevArr<int64_t> d_ao(ann_off.size() * 8, ann_off.data());
	DevArr<double> d_tab(tab.size() * 8, tab.data());
	DevArr<AlnReq> d_rq(n * sizeof(AlnReq));
	DevArr<SamDesc> d_ds(n * sizeof(SamDesc));
	launch_pair_simple(0, pp, n_pairs, d_first, d_nf, d_ok, d_ao, d_aa, d_tab, d_tab + n_tab, d_st, d_rq, d_ds);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	d_st.download(status, n_pairs);
	d_ds.download(desc, n * sizeof(SamDesc));
	d_rq.download(req, n * sizeof(AlnReq));
	return 0;
}

// The same kernel for the designed stage test (tests/test_gpu_pair_stage.py): the caller also gives the pair_ok bytes (0: a pair the
// host did not pass), and status, desc and req come back WHOLE — room for mi355x_pair_stage_room(n_pairs) pairs (n_pairs rounded up to
// the workgroup, and one workgroup more), every byte `fill` before the launch — so that the caller sees what the kernel wrote and
// what it left alone, behind the last pair too.
extern "C" int mi355x_pair_stage_room(int n_pairs) { return n_pairs <= 0 ? 0 : (n_pairs + 63) / 64 * 64 + 64; }
extern "C" int mi355x_pair_stage_batch(const mem_opt_t *opt, const bntseq_t *bns, const mem_pestat_t pes[4], int64_t n_processed, int n_pairs,
                                       const void *regs, const int *n_regs, const uint8_t *pair_ok, int max_len, int fill, uint8_t *status,
                                       void *desc, void *req)
{
	require_any_device();
	if (n_pairs <= 0) return 0;
	if (max_len <= 0) die("mi355x_pair_stage_batch: max_len must be positive");
	PairParams pp;
	size_t n_tab = 0;
	if (!pair_params(opt, bns->l_pac, pes, n_processed, max_len, pp, &n_tab)) return -1;
	std::vector<double> tab(n_tab + (size_t)pp.ltab_n);
	pair_tables(opt, pes, pp, n_tab, tab.data());
	std::vector<int64_t> ann_off;
	std::vector<uint8_t> ann_alt;
	contig_table(bns, ann_off, ann_alt);
	const size_t n = (size_t)2 * n_pairs, room = (size_t)mi355x_pair_stage_room(n_pairs);
	const DevReg *hr = (const DevReg *)regs;
	for (size_t i = 0; i < n; ++i)   // nothing the kernel indexes with may point outside what is uploaded
		for (int j = 0; j < n_regs[i] && j < PR_MAXREG; ++j)
			if (hr[i * PR_MAXREG + j].rid < 0 || hr[i * PR_MAXREG + j].rid >= bns->n_seqs) die("mi355x_pair_stage_batch: bad contig in region %d of read %zu", j, i);
	DevArr<DevReg> d_first(n * PR_MAXREG * sizeof(DevReg), regs);
	DevArr<int> d_nf(n * 4, n_regs);
	DevArr<uint8_t> d_ok(n_pairs, pair_ok), d_aa(ann_alt.size(), ann_alt.data()), d_st(room);
	DevArr<int64_t> d_ao(ann_off.size() * 8, ann_off.data());
	DevArr<double> d_tab(tab.size() * 8, tab.data());
	DevArr<AlnReq> d_rq(2 * room * sizeof(AlnReq));
	DevArr<SamDesc> d_ds(2 * room * sizeof(SamDesc));
	d_st.fill(fill); d_rq.fill(fill); d_ds.fill(fill);
	launch_pair_simple(0, pp, n_pairs, d_first, d_nf, d_ok, d_ao, d_aa, d_tab, d_tab + n_tab, d_st, d_rq, d_ds);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	d_st.download(status, room);
	d_ds.download(desc, 2 * room * sizeof(SamDesc));
	d_rq.download(req, 2 * room * sizeof(AlnReq));
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
// the record of a mate-rescue request that the device does not answer
static MswRes msw_host_request()
{
	MswRes r;
	r.score = 0; r.te = r.qe = r.score2 = r.te2 = r.tb = r.qb = -1; r.flags = 1;
	return r;
}
static int pair_wave_batch(const char *who, const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], int64_t n_processed,
                           int n_pairs, const uint8_t *reads, const int64_t *off, const void *regs, const int *reg_off, uint8_t *status,
                           void *desc, void *req, int *n_align, void *xa_req, uint8_t *xa_cnt, uint8_t *n_lines = nullptr, void *line_desc = nullptr,
                           void *line_req = nullptr, uint8_t *line_xa_cnt = nullptr, void *line_xa_req = nullptr)
{
	require_any_device();
	if (n_align) *n_align = 0;
	if (n_pairs <= 0) return 0;
	if (n_lines && (!line_desc || !line_req || !line_xa_cnt)) die("%s: no room for the lines", who);
	const int n_reads = 2 * n_pairs;
	const size_t n_slots = (size_t)n_reads * SE_LINES_CAP;
	if (n_lines) {
		memset(n_lines, 0, (size_t)n_reads);
		memset(line_xa_cnt, 0, n_slots);
		memset(line_desc, 0xff, n_slots * sizeof(SamDesc));
		memset(line_req, 0xff, n_slots * sizeof(AlnReq));
		if (line_xa_req) memset(line_xa_req, 0xff, n_slots * PW_XA_CAP * sizeof(AlnReq));
	}
	memset(status, 0, (size_t)n_pairs);
	memset(desc, 0xff, (size_t)n_reads * sizeof(SamDesc));
	memset(req, 0xff, (size_t)n_reads * sizeof(AlnReq));
	if (xa_req) { memset(xa_req, 0xff, (size_t)n_reads * PW_XA_CAP * sizeof(AlnReq)); memset(xa_cnt, 0, (size_t)n_reads); }
	// (the calls whose pairs are all the host's, as for pair_simple_kernel: -P, -a, -V, -5, mapQ_coef_len 0)
	if ((opt->flag & (MEM_F_NOPAIRING | MEM_F_ALL | MEM_F_REF_HDR | MEM_F_PRIMARY5)) || !(opt->mapQ_coef_len > 0)) return 0;
	const int64_t l_pac = bns->l_pac;
	const PackedReads R = pack_reads(n_reads, reads, off, 4);
	const std::vector<int> &lens = R.lens;
	const int max_len = std::max(R.max_len, 1);
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
		if (!ok || !pair_wave_eligible(a, PW_MAXREG, n_lines != nullptr)) continue;
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
	// ---- device: every array with PAD bytes behind what it holds ----
	hipStream_t st = 0;
	const size_t PAD = 64, nw = (size_t)n_work;
	int max_t = 1;
	for (size_t i = 0; i < n_mreq; ++i) max_t = std::max(max_t, (int)(mreq[i].re - mreq[i].rb));
	DevArr<uint8_t> d_seq(R.flat.size() + PAD, R.flat.data(), R.flat.size()), d_pac((size_t)(l_pac / 4 + 1) + PAD, pac, (size_t)(l_pac / 4 + 1));
	DevArr<int64_t> d_off((size_t)(n_reads + 1) * 8 + PAD, R.slot.data(), (size_t)(n_reads + 1) * 8);
	DevArr<int> d_len((size_t)n_reads * 4 + PAD, lens.data(), (size_t)n_reads * 4);
	DevArr<MswReq> d_mreq(n_mreq * sizeof(MswReq) + PAD, mreq.data(), n_mreq * sizeof(MswReq));
	DevArr<MswRes> d_mres(n_mreq * sizeof(MswRes) + PAD);
	DevArr<uint16_t> d_rows;
	DevArr<int> d_list, d_tail;
	if (n_mreq) {
		d_rows = DevArr<uint16_t>(n_mreq * (size_t)max_t * 2 + PAD);
		std::vector<int> h_list(2 * n_mreq + 16);
		d_list = DevArr<int>((2 * n_mreq + 16) * sizeof(int) + PAD);
		d_tail = DevArr<int>(msw_tail_ints(n_mreq) * sizeof(int) + PAD);
		if (msw_on_device(opt)) {
			launch_msw(st, msw_params(opt, l_pac), (int)n_mreq, d_mreq, d_seq, d_off, d_len, d_pac, d_mres, d_rows, max_len, (const MswReq *)mreq.data(),
			           lens.data(), h_list.data(), d_list, d_tail);
			HIP_OK(hipStreamSynchronize(st));   // (h_list is read by the copy queued in launch_msw)
		} else {   // options the kernels do not take: every request is the host's (flags = 1), as the pipeline would have kept them all
			const std::vector<MswRes> back(n_mreq, msw_host_request());
			HIP_OK(hipMemcpy(d_mres, back.data(), n_mreq * sizeof(MswRes), hipMemcpyHostToDevice));
		}
	}
	DevArr<int> d_work(nw * 4 + PAD, work.data(), nw * 4);
	DevArr<DevReg> d_lists(lists.size() * sizeof(DevReg) + PAD, lists.data(), lists.size() * sizeof(DevReg));
	DevArr<int> d_loff(loff.size() * 4 + PAD, loff.data(), loff.size() * 4);
	DevArr<unsigned> d_mfirst(mfirst.size() * 4 + PAD, mfirst.data(), mfirst.size() * 4);
	DevArr<short> d_tags(tags.size() * 2 + PAD, tags.data(), tags.size() * 2);
	DevArr<int> d_toff(toff.size() * 4 + PAD, toff.data(), toff.size() * 4);
	DevArr<int64_t> d_ao(ann_off.size() * 8 + PAD, ann_off.data(), ann_off.size() * 8);
	DevArr<double> d_tab(tab.size() * 8 + PAD, tab.data(), tab.size() * 8);
	DevArr<uint8_t> d_ws(nw + PAD), d_xc;
	DevArr<AlnReq> d_rq(2 * nw * sizeof(AlnReq) + PAD), d_xr;
	DevArr<SamDesc> d_ds(2 * nw * sizeof(SamDesc) + PAD);
	if (xa_req) {
		d_xr = DevArr<AlnReq>(2 * nw * PW_XA_CAP * sizeof(AlnReq) + PAD);
		d_xc = DevArr<uint8_t>(2 * nw + PAD);
	}
	d_ws.fill(0, nw);
	if (d_xc) d_xc.fill(0, 2 * nw);
	const size_t nl = 2 * nw * SE_LINES_CAP;   // the side arrays by (work item, end, line)
	DevArr<uint8_t> d_ln, d_lxc;
	DevArr<SamDesc> d_lds;
	DevArr<AlnReq> d_lrq, d_lxr;
	SeLines LN;
	if (n_lines) {
		d_ln = DevArr<uint8_t>(2 * nw + PAD); d_lxc = DevArr<uint8_t>(nl + PAD);
		d_lds = DevArr<SamDesc>(nl * sizeof(SamDesc) + PAD);
		d_lrq = DevArr<AlnReq>(nl * sizeof(AlnReq) + PAD);
		d_ln.fill(0, 2 * nw); d_lxc.fill(0, nl);
		d_lds.fill(0xff, nl * sizeof(SamDesc));
		d_lrq.fill(0xff, nl * sizeof(AlnReq));
		LN.desc = d_lds; LN.reqs = d_lrq; LN.n_lines = d_ln; LN.xa_cnt = d_lxc;
		if (line_xa_req) {
			d_lxr = DevArr<AlnReq>(nl * PW_XA_CAP * sizeof(AlnReq) + PAD);
			d_lxr.fill(0xff, nl * PW_XA_CAP * sizeof(AlnReq));
			LN.xa_reqs = d_lxr;
		}
		se_lines_options(opt, LN);
	}
	launch_pair_wave(st, pp, n_work, d_work, d_lists, d_loff, d_len, d_mreq, d_mres, d_mfirst, d_tags, d_toff, d_ao, d_tab, d_tab + n_tab, d_ws, d_rq, d_ds,
	                 d_xr, d_xc, n_lines ? &LN : nullptr);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	std::vector<uint8_t> ws(nw);
	d_ws.download(ws.data(), nw);
	std::vector<SamDesc> w_ds(2 * nw);
	std::vector<AlnReq> w_rq(2 * nw);
	d_ds.download(w_ds.data(), w_ds.size() * sizeof(SamDesc));
	d_rq.download(w_rq.data(), w_rq.size() * sizeof(AlnReq));
	std::vector<AlnReq> w_xr(xa_req ? 2 * nw * PW_XA_CAP : 0);
	std::vector<uint8_t> w_xc(xa_req ? 2 * nw : 0);
	if (xa_req) {
		d_xr.download(w_xr.data(), w_xr.size() * sizeof(AlnReq));
		d_xc.download(w_xc.data(), w_xc.size());
	}
	std::vector<uint8_t> w_ln(n_lines ? 2 * nw : 0), w_lxc(n_lines ? nl : 0);
	std::vector<SamDesc> w_lds(n_lines ? nl : 0);
	std::vector<AlnReq> w_lrq(n_lines ? nl : 0), w_lxr(line_xa_req ? nl * PW_XA_CAP : 0);
	if (n_lines) {
		d_ln.download(w_ln.data(), w_ln.size());
		d_lxc.download(w_lxc.data(), w_lxc.size());
		d_lds.download(w_lds.data(), w_lds.size() * sizeof(SamDesc));
		d_lrq.download(w_lrq.data(), w_lrq.size() * sizeof(AlnReq));
		if (line_xa_req) d_lxr.download(w_lxr.data(), w_lxr.size() * sizeof(AlnReq));
	}
	for (int t = 0; t < n_work; ++t) {
		status[work[t]] = ws[t];
		if (ws[t] == PW_DECIDED_LINES && n_lines)
			for (int e = 0; e < 2; ++e) {   // slot (2t + e, line) of the work list -> slot (2 work[t] + e, line) of the call
				const size_t from = (size_t)(2 * t + e) * SE_LINES_CAP, to = (size_t)(2 * work[t] + e) * SE_LINES_CAP;
				const int c = std::min<int>(w_ln[2 * t + e], SE_LINES_CAP);
				n_lines[2 * work[t] + e] = (uint8_t)c;
				for (int j = 0; j < c; ++j) {
					const int x = std::min<int>(w_lxc[from + j], PW_XA_CAP);
					((SamDesc *)line_desc)[to + j] = w_lds[from + j];
					((AlnReq *)line_req)[to + j] = w_lrq[from + j];
					line_xa_cnt[to + j] = (uint8_t)x;
					if (line_xa_req) memcpy((AlnReq *)line_xa_req + (to + j) * PW_XA_CAP, &w_lxr[(from + j) * PW_XA_CAP], (size_t)x * sizeof(AlnReq));
				}
			}
		if (ws[t] != PR_DECIDED && ws[t] != PW_DECIDED_XA) continue;
		for (int e = 0; e < 2; ++e) { ((SamDesc *)desc)[2 * work[t] + e] = w_ds[2 * t + e]; ((AlnReq *)req)[2 * work[t] + e] = w_rq[2 * t + e]; }
		if (ws[t] != PW_DECIDED_XA) continue;
		for (int e = 0; e < 2; ++e) {
			const int c = std::min<int>(w_xc[2 * t + e], PW_XA_CAP);
			xa_cnt[2 * work[t] + e] = (uint8_t)c;
			memcpy((AlnReq *)xa_req + (size_t)(2 * work[t] + e) * PW_XA_CAP, &w_xr[(size_t)(2 * t + e) * PW_XA_CAP], (size_t)c * sizeof(AlnReq));
		}
	}
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
// The same with the side arrays for the pairs mem_sam_pe reports end by end through no_pairing: (status 17, PW_DECIDED_LINES; device.h):
// n_lines[2k + e] lines of end e (0: the unaligned record), and by (read 2k + e, line) = slot (2k + e) * mi355x_se_lines_cap() + line
// line_desc, line_req, line_xa_cnt and line_xa_req (mi355x_pair_wave_xa_cap() requests each).  A pair without any region is handed to
// the kernel too.  xa_req = NULL: without the XA listing of the paired branch; line_xa_req = NULL: without that of the lines.
extern "C" int mi355x_pair_wave_lines_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], int64_t n_processed,
                                            int n_pairs, const uint8_t *reads, const int64_t *off, const void *regs, const int *reg_off, uint8_t *status,
                                            void *desc, void *req, int *n_align, void *xa_req, uint8_t *xa_cnt, uint8_t *n_lines, void *line_desc,
                                            void *line_req, uint8_t *line_xa_cnt, void *line_xa_req)
{
	if (xa_req && !xa_cnt) die("mi355x_pair_wave_lines_batch: no room for the XA counts");
	if (!n_lines) die("mi355x_pair_wave_lines_batch: no room for the line counts");
	return pair_wave_batch("mi355x_pair_wave_lines_batch", opt, bns, pac, pes, n_processed, n_pairs, reads, off, regs, reg_off, status, desc, req, n_align,
	                       xa_req, xa_req ? xa_cnt : nullptr, n_lines, line_desc, line_req, line_xa_cnt, line_xa_req);
}

// Stage entry of se_wave_kernel (se_wave_kernel.hip) for parity tests: n_work single-end reads given by their numbers in the chunk
// (read_no[t]: id = n_processed + read_no[t], req.read = read_no[t]) and their regions as they stand after mem_sort_dedup_patch (regs:
// DevReg records back to back, reg_off[n_work + 1]), through the pipeline's own launch function.  Everything is by work item t:
// status[t] = 1 (SE_DECIDED): desc[t] (SamDesc) and req[t] (AlnReq; none for the unmapped record) are what mem_reg2sam reports with one
// plain line; SE_DECIDED_XA (xa_req given): the line carries an XA tag of xa_cnt[t] entries, their requests at xa_req[t * PW_XA_CAP ..]
// (pad = the entry's contig), the count also in desc[t].flag bits 16-19; else the code of the test that left the read to the host
// (device.h: SE_HOST_*), desc[t].req = req[t].read = -1.  xa_req = NULL: without the XA listing.
// n_lines given (mi355x_se_wave_lines_batch): the kernel runs with the side arrays of device.h: SeLines, all of them by (t, line) = slot
// t * SE_LINES_CAP + line; line_xa_req = NULL: without the XA listing of the lines.
extern "C" int mi355x_se_lines_cap(void) { return SE_LINES_CAP; }
static int se_wave_batch(const char *who, const mem_opt_t *opt, const bntseq_t *bns, int64_t n_processed, int n_work, const int *read_no, const void *regs,
                         const int *reg_off, int max_len, uint8_t *status, void *desc, void *req, uint8_t *xa_cnt, void *xa_req, uint8_t *n_lines,
                         void *line_desc, void *line_req, uint8_t *line_xa_cnt, void *line_xa_req)
{
	require_any_device();
	if (n_work <= 0) return 0;
	if (max_len <= 0) die("%s: max_len must be positive", who);
	if (xa_req && !xa_cnt) die("%s: no room for the XA counts", who);
	if (n_lines && (!line_desc || !line_req || !line_xa_cnt)) die("%s: no room for the lines", who);
	const size_t nw = (size_t)n_work;
	memset(status, 0, nw);
	memset(desc, 0xff, nw * sizeof(SamDesc));
	memset(req, 0xff, nw * sizeof(AlnReq));
	if (xa_cnt) memset(xa_cnt, 0, nw);
	if (xa_req) memset(xa_req, 0xff, nw * PW_XA_CAP * sizeof(AlnReq));
	// nothing the kernel indexes with may point outside what is uploaded
	if (reg_off[0] != 0) die("%s: reg_off[0] must be 0", who);
	for (size_t t = 0; t < nw; ++t) {
		if (reg_off[t + 1] < reg_off[t]) die("%s: reg_off decreases at work item %zu", who, t);
		if (read_no[t] < 0) die("%s: bad read number at work item %zu", who, t);
	}
	const size_t NR = (size_t)reg_off[nw];
	const DevReg *hr = (const DevReg *)regs;
	for (size_t j = 0; j < NR; ++j)
		if (hr[j].rid < 0 || hr[j].rid >= bns->n_seqs) die("%s: bad contig in region %zu", who, j);
	PairParams pp;
	mem_pestat_t pes[4];
	se_params(opt, bns->l_pac, n_processed, max_len, pp, pes);
	std::vector<double> tab((size_t)pp.ltab_n);
	pair_tables(opt, pes, pp, 0, tab.data());
	std::vector<int64_t> ann_off;
	std::vector<uint8_t> ann_alt;
	contig_table(bns, ann_off, ann_alt);
	const size_t PAD = 64;
	DevArr<int> d_work(nw * 4 + PAD, read_no, nw * 4), d_loff((nw + 1) * 4 + PAD, reg_off, (nw + 1) * 4);
	DevArr<DevReg> d_lists(NR * sizeof(DevReg) + PAD, regs, NR * sizeof(DevReg));
	DevArr<uint8_t> d_aa(ann_alt.size() + PAD, ann_alt.data(), ann_alt.size()), d_ws(nw + PAD), d_xc;
	DevArr<double> d_tab(tab.size() * 8 + PAD, tab.data(), tab.size() * 8);
	DevArr<AlnReq> d_rq(nw * sizeof(AlnReq) + PAD), d_xr;
	DevArr<SamDesc> d_ds(nw * sizeof(SamDesc) + PAD);
	d_ws.fill(0, nw);
	d_rq.fill(0xff, nw * sizeof(AlnReq));
	d_ds.fill(0xff, nw * sizeof(SamDesc));
	if (xa_req) {
		d_xr = DevArr<AlnReq>(nw * PW_XA_CAP * sizeof(AlnReq) + PAD);
		d_xc = DevArr<uint8_t>(nw + PAD);
		d_xr.fill(0xff, nw * PW_XA_CAP * sizeof(AlnReq));
		d_xc.fill(0, nw);
	}
	const size_t nl = nw * SE_LINES_CAP;
	DevArr<uint8_t> d_ln, d_lxc;
	DevArr<SamDesc> d_lds;
	DevArr<AlnReq> d_lrq, d_lxr;
	SeLines LN;
	if (n_lines) {
		d_ln = DevArr<uint8_t>(nw + PAD); d_lxc = DevArr<uint8_t>(nl + PAD);
		d_lds = DevArr<SamDesc>(nl * sizeof(SamDesc) + PAD);
		d_lrq = DevArr<AlnReq>(nl * sizeof(AlnReq) + PAD);
		d_ln.fill(0, nw); d_lxc.fill(0, nl);
		d_lds.fill(0xff, nl * sizeof(SamDesc));
		d_lrq.fill(0xff, nl * sizeof(AlnReq));
		LN.desc = d_lds; LN.reqs = d_lrq; LN.n_lines = d_ln; LN.xa_cnt = d_lxc;
		if (line_xa_req) {
			d_lxr = DevArr<AlnReq>(nl * PW_XA_CAP * sizeof(AlnReq) + PAD);
			d_lxr.fill(0xff, nl * PW_XA_CAP * sizeof(AlnReq));
			LN.xa_reqs = d_lxr;
		}
		se_lines_options(opt, LN);
	}
	launch_se_wave(0, pp, n_work, d_work, d_lists, d_loff, d_aa, d_tab, d_ws, d_rq, d_ds, d_xr, d_xc, n_lines ? &LN : nullptr);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	d_ws.download(status, nw);
	d_ds.download(desc, nw * sizeof(SamDesc));
	d_rq.download(req, nw * sizeof(AlnReq));
	if (xa_req) {
		d_xr.download(xa_req, nw * PW_XA_CAP * sizeof(AlnReq));
		d_xc.download(xa_cnt, nw);
	}
	if (n_lines) {
		d_ln.download(n_lines, nw);
		d_lxc.download(line_xa_cnt, nl);
		d_lds.download(line_desc, nl * sizeof(SamDesc));
		d_lrq.download(line_req, nl * sizeof(AlnReq));
		if (line_xa_req) d_lxr.download(line_xa_req, nl * PW_XA_CAP * sizeof(AlnReq));
	}
	return 0;
}
extern "C" int mi355x_se_wave_batch(const mem_opt_t *opt, const bntseq_t *bns, int64_t n_processed, int n_work, const int *read_no, const void *regs,
                                    const int *reg_off, int max_len, uint8_t *status, void *desc, void *req, uint8_t *xa_cnt, void *xa_req)
{
	return se_wave_batch("mi355x_se_wave_batch", opt, bns, n_processed, n_work, read_no, regs, reg_off, max_len, status, desc, req, xa_cnt, xa_req, nullptr,
	                     nullptr, nullptr, nullptr, nullptr);
}
// The same with the side arrays for reads of 2 .. mi355x_se_lines_cap() lines (status 17, SE_DECIDED_LINES): n_lines[t], and by
// (t, line) line_desc, line_req, line_xa_cnt and line_xa_req (mi355x_pair_wave_xa_cap() requests each).  n_lines = NULL: exactly
// mi355x_se_wave_batch.
extern "C" int mi355x_se_wave_lines_batch(const mem_opt_t *opt, const bntseq_t *bns, int64_t n_processed, int n_work, const int *read_no, const void *regs,
                                          const int *reg_off, int max_len, uint8_t *status, void *desc, void *req, uint8_t *xa_cnt, void *xa_req,
                                          uint8_t *n_lines, void *line_desc, void *line_req, uint8_t *line_xa_cnt, void *line_xa_req)
{
	return se_wave_batch("mi355x_se_wave_lines_batch", opt, bns, n_processed, n_work, read_no, regs, reg_off, max_len, status, desc, req, xa_cnt, xa_req,
	                     n_lines, line_desc, line_req, line_xa_cnt, line_xa_req);
}

extern "C" int mi355x_smem_batch(const mem_opt_t *opt, int n, const uint8_t *seqs, const int64_t *off, int cap,
                                 uint64_t *intv_out, int *n_out, double *kernel_ms, uint64_t *algo_bytes)
{
	need_index();
	if (n <= 0) return 0;
	hipStream_t st = 0;
	const PackedReads R = pack_reads(n, seqs, off, 0);   // 16-byte aligned slots, as the kernel expects
	const int max_len = R.max_len;
	size_t total = off[n];
	size_t per_quad = 0;
	int n_quads = smem_grid_quads(max_len, &per_quad);
	DevArr<uint8_t> d_seq(R.flat.size(), R.flat.data());
	DevArr<int> d_len((size_t)n * 4, R.lens.data()), d_nout((size_t)n * 4);
	DevArr<int64_t> d_off((size_t)(n + 1) * 8, R.slot.data());
	DevArr<uint64_t> d_out((size_t)n * cap * 32);
	DevArr<unsigned long long> d_cnt(256);
	DevArr<void> d_scr(per_quad * n_quads);
	d_cnt.zero();
	d_nout.zero();
	Timer tm;
	tm.start(st);
	const char *ce = getenv("MPIBWA_SMEM_COUNT");   // "0": the production variant of passes 1-2 (no block counting; *algo_bytes = 0)
	const bool count_blocks = !(ce && atoi(ce) == 0);
	launch_smem(st, dev_index().fm, smem_params(opt), n, d_seq, d_off, d_len, cap, d_out, d_nout, max_len, d_cnt, d_scr, per_quad, n_quads, count_blocks);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	unsigned long long cnt[32];
	d_cnt.download(cnt, 256);
	d_nout.download(n_out, (size_t)n * 4);
	d_out.download(intv_out, (size_t)n * cap * 32);
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

extern "C" int mi355x_sa_batch(int n, const uint64_t *k, uint64_t *sa_out, double *kernel_ms, uint64_t *algo_bytes)
{
	need_index();
	if (n <= 0) return 0;
	hipStream_t st = 0;
	DevArr<uint64_t> d_k((size_t)n * 8, k), d_o((size_t)n * 8);
	DevArr<unsigned long long> d_cnt(64);
	d_cnt.zero();
	Timer tm;
	tm.start(st);
	launch_sa(st, dev_index().fm, n, d_k, d_o, d_cnt);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	unsigned long long cnt[8];
	d_cnt.download(cnt, 64);
	d_o.download(sa_out, (size_t)n * 8);
	if (kernel_ms) *kernel_ms = ms;
	if (algo_bytes) *algo_bytes = cnt[1] * 64 + (uint64_t)n * 8;   // 64 B per LF step + the sampled SA word
	return 0;
}

// dense != 0: answer from the expanded table (fails if it is absent); dense == 0: LF walk on the sampled SA
extern "C" int mi355x_sa_batch2(int n, const uint64_t *k, uint64_t *sa_out, double *kernel_ms, int dense)
{
	need_index();
	if (!dense) return mi355x_sa_batch(n, k, sa_out, kernel_ms, nullptr);
	if (!dev_index().fm.sa_full) return -1;
	if (n <= 0) return 0;
	DevArr<uint64_t> d_k((size_t)n * 8, k), d_o((size_t)n * 8);
	Timer tm;
	tm.start(0);
	launch_sa_dense(0, dev_index().fm, n, d_k, d_o);
	double ms = tm.stop(0);
	HIP_OK(hipGetLastError());
	d_o.download(sa_out, (size_t)n * 8);
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}
extern "C" double mi355x_sa_dense_info(size_t *bytes) { if (bytes) *bytes = dev_index().sa_full_bytes; return dev_index().sa_expand_ms; }

// mi355x_extend_batch (per_job = false: launch_extend, no early / clip, *cells = the total) and mi355x_extend_batch2 (per_job = true:
// launch_extend2 with early[] and clip[], cells[] = one count per job)
static int extend_batch(const mem_opt_t *opt, int n, const uint8_t *q, const int64_t *qoff, const uint8_t *t, const int64_t *toff, const int *w,
                        const int *h0, const int *end_bonus, const int *early, const int *clip, bool per_job, int *out6, uint64_t *cells,
                        double *kernel_ms)
{
	require_any_device();
	if (n <= 0) return 0;
	hipStream_t st = 0;
	std::vector<int> wc(n);
	int max_qlen = 0;
	for (int i = 0; i < n; ++i) {
		int ql = (int)(qoff[i + 1] - qoff[i]);
		max_qlen = std::max(max_qlen, ql);
		wc[i] = clamp_band(opt, ql, w[i], end_bonus[i]);
	}
	const size_t n4 = (size_t)n * 4, cell_bytes = per_job ? (size_t)n * 8 : 8;
	DevArr<uint8_t> d_q(qoff[n] + 16, q, qoff[n]), d_t(toff[n] + 16, t, toff[n]);
	DevArr<int64_t> d_qo((size_t)(n + 1) * 8, qoff), d_to((size_t)(n + 1) * 8, toff);
	DevArr<int> d_w(n4, wc.data()), d_h0(n4, h0), d_early, d_clip, d_out((size_t)n * 24);
	if (per_job) { d_early = DevArr<int>(n4, early); d_clip = DevArr<int>(n4, clip); }
	DevArr<unsigned long long> d_cells(cell_bytes);
	d_cells.zero();
	const ExtParams ep = ext_params(opt);
	Timer tm;
	tm.start(st);
	if (per_job) launch_extend2(st, ep, n, d_q, d_qo, d_t, d_to, d_w, d_h0, d_early, d_clip, d_out, d_cells, max_qlen);
	else launch_extend(st, ep, n, d_q, d_qo, d_t, d_to, d_w, d_h0, nullptr, d_out, d_cells, max_qlen);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	unsigned long long c = 0;
	d_cells.download(per_job ? (void *)cells : &c, cell_bytes);
	d_out.download(out6, (size_t)n * 24);
	if (kernel_ms) *kernel_ms = ms;
	if (!per_job && cells) *cells = c;
	return 0;
}
extern "C" int mi355x_extend_batch(const mem_opt_t *opt, int n, const uint8_t *q, const int64_t *qoff, const uint8_t *t,
                                   const int64_t *toff, const int *w, const int *h0, const int *end_bonus, int *out6,
                                   double *kernel_ms, uint64_t *cells)
{
	return extend_batch(opt, n, q, qoff, t, toff, w, h0, end_bonus, nullptr, nullptr, false, out6, cells, kernel_ms);
}
extern "C" int mi355x_extend_batch2(const mem_opt_t *opt, int n, const uint8_t *q, const int64_t *qoff, const uint8_t *t,
                                    const int64_t *toff, const int *w, const int *h0, const int *end_bonus, const int *early,
                                    const int *clip, int *out6, uint64_t *cells, double *kernel_ms)
{
	return extend_batch(opt, n, q, qoff, t, toff, w, h0, end_bonus, early, clip, true, out6, cells, kernel_ms);
}

// Stage-level entry point of the mate-rescue alignment (tests, micro-benchmarks): n_req windows [rb,re) of the packed
// reference `pac` (doubled coordinate, 2 bits per base, l_pac bases) against reads of a batch given as nt4 codes.
// out8 per request: score, te, qe, score2, te2, tb, qb, flags — kswr_t of ksw_align2 with mem_matesw's flags.
// what the second pass of the last mi355x_matesw_batch ran: pairs, alone-riders, work items of a register launch, of the general launch
static uint64_t g_matesw_counts[4];
extern "C" void mi355x_matesw_batch_counts(uint64_t out[4])
{
	for (int i = 0; i < 4; ++i) out[i] = g_matesw_counts[i];
}

extern "C" int mi355x_matesw_batch(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, int n_reads, const uint8_t *reads, const int64_t *off,
                                   int n_req, const int64_t *rb, const int64_t *re, const int *read, const int *is_rev, int *out8,
                                   double *kernel_ms)
{
	require_any_device();
	for (int i = 0; i < 4; ++i) g_matesw_counts[i] = 0;
	if (n_req <= 0) return 0;
	static_assert(sizeof(MswRes) == 32, "MswRes layout");
	if (!msw_on_device(opt)) {   // options the kernels do not take: every request is handed back (flags = 1: recompute on the host)
		const MswRes back = msw_host_request();
		for (int i = 0; i < n_req; ++i) memcpy(out8 + 8 * (size_t)i, &back, sizeof(MswRes));
		if (kernel_ms) *kernel_ms = 0;
		return 0;
	}
	hipStream_t st = 0;
	const PackedReads R = pack_reads(n_reads, reads, off, 4);   // reads go into 16-byte slots as in the pipeline
	const int max_len = R.max_len;
	if ((int64_t)max_len * opt->a >= 8192 || msw_lds_bytes(max_len) > 160 * 1024) die("mate-rescue kernel: reads too long for the device path");
	std::vector<MswReq> rq(n_req);
	int max_t = 1;
	for (int i = 0; i < n_req; ++i) {
		rq[i].rb = rb[i]; rq[i].re = re[i]; rq[i].read = read[i]; rq[i].is_rev = is_rev[i];
		if (re[i] < rb[i] || re[i] > 2 * l_pac || rb[i] < 0 || read[i] < 0 || read[i] >= n_reads) die("mi355x_matesw_batch: bad request %d", i);
		max_t = std::max(max_t, (int)(re[i] - rb[i]));
	}
	DevArr<uint8_t> d_seq(R.flat.size(), R.flat.data()), d_pac(l_pac / 4 + 16, pac, l_pac / 4 + 1);
	DevArr<int64_t> d_off((size_t)(n_reads + 1) * 8, R.slot.data());
	DevArr<int> d_len((size_t)n_reads * 4, R.lens.data());
	DevArr<MswReq> d_req((size_t)n_req * sizeof(MswReq), rq.data());
	DevArr<MswRes> d_res((size_t)n_req * sizeof(MswRes));
	DevArr<uint16_t> d_rows((size_t)n_req * max_t * 2);
	std::vector<int> h_list(2 * (size_t)n_req + 16);
	DevArr<int> d_list((2 * (size_t)n_req + 16) * sizeof(int)), d_tail(msw_tail_ints(n_req) * sizeof(int));
	d_tail.fill(0, 2 * MSW_OFF_INTS * sizeof(int));   // (a call without a packed launch leaves the class offsets alone: nothing ran)
	Timer tm;
	tm.start(st);
	launch_msw(st, msw_params(opt, l_pac), n_req, d_req, d_seq, d_off, d_len, d_pac, d_res, d_rows, max_len, rq.data(), R.lens.data(), h_list.data(), d_list,
	           d_tail);
	double ms = tm.stop(st);
	HIP_OK(hipGetLastError());
	msw_tail_counts(d_tail, g_matesw_counts);
	d_res.download(out8, (size_t)n_req * sizeof(MswRes));
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
		require_any_device();
		std::vector<int64_t> ann_off;
		std::vector<uint8_t> ann_alt;
		contig_table(bns, ann_off, ann_alt);
		const size_t n4 = (size_t)n_reads * 4, s8 = (size_t)S * 8;
		DevArr<int> d_len(n4 + 4, lens, n4), d_ns(n4 + 4, nseeds.data(), n4), d_lrep(n4 + 4, l_rep, n4), d_tab(tab.size() * 4, tab.data()), d_nch(n4 + 4);
		DevArr<int64_t> d_so((size_t)(n_reads + 1) * 8, seed_off), d_ao(ann_off.size() * 8, ann_off.data());
		DevArr<uint8_t> d_aa(ann_alt.size(), ann_alt.data());
		DevArr<uint64_t> d_sa(s8 + 8, rbeg, s8);
		DevArr<int32_t> d_qbl(s8 + 8, qbeg_len, s8);
		DevArr<DevChain> d_ch((size_t)(S + 1) * sizeof(DevChain));
		DevArr<DevSeed> d_sd((size_t)(S + 1) * sizeof(DevSeed));
		DevArr<unsigned int> d_srt((size_t)(S + 1) * 4);
		DevArr<void> d_scr(chain_scratch_bytes(n_reads));
		launch_chain(0, chain_params(opt, bns->l_pac), n_reads, d_len, d_ns, d_lrep, d_so, d_sa, d_qbl, d_ao, d_aa, bns->n_seqs, d_tab, TS, d_ch, d_sd, d_srt, d_nch, d_scr);
		HIP_OK(hipDeviceSynchronize());
		d_nch.download(nch.data(), n4);
		d_ch.download((void *)chains.data(), (size_t)S * sizeof(DevChain));
		d_sd.download((void *)seeds.data(), (size_t)S * sizeof(DevSeed));
	} else {
		// the pipeline's host chaining of a read (without mem_flt_chained_seeds: no reads here), its run moved to the slots from seed_off[i]
		HostChainer hc;
		std::vector<DevChain> och;
		std::vector<DevSeed> osd;
		for (int i = 0; i < n_reads; ++i) {
			const int64_t so = seed_off[i];
			och.clear(); osd.clear();
			nch[i] = host_chain_read(opt, bns, nullptr, lens[i], nullptr, rbeg + so, qbeg_len + 2 * so, nseeds[i], l_rep[i], tab.data(), hc, och, osd);
			for (int c = 0; c < nch[i]; ++c) { chains[so + c] = och[c]; chains[so + c].seed_beg += (int)so; }
			std::copy(osd.begin(), osd.end(), seeds.begin() + so);
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
// pipeline's sequence: the length tables, the launch order, the chain groups with their round trip, and the pipeline's own queue_c2a().
extern "C" int64_t mi355x_c2a_batch(const mem_opt_t *opt, const bntseq_t *bns, int n_reads, const uint8_t *reads, const int64_t *off,
                                    const int *n_chains, const int *chain_rid, const float *chain_frac, const int *chain_nseeds,
                                    const int64_t *seed_rbeg, const int *seed_qbeg, const int *seed_len, const int *seed_score,
                                    int heavy_t, int early, int layout, int64_t *out, int64_t out_cap, int64_t *out_off,
                                    uint64_t *stat4, int *n_units)
{
	need_index();
	if (bns->l_pac != dev_index().l_pac) die("mi355x_c2a_batch: the index given is not the resident one");
	if (layout != 0 && layout != 1) die("mi355x_c2a_batch: layout %d", layout);
	if (n_reads <= 0) return 0;
	const int64_t l_pac = bns->l_pac;
	// the reads in 16-byte slots, 16 bytes of padding behind the last one (the kernel stages a read 4 bytes at a time)
	const PackedReads R = pack_reads(n_reads, reads, off, 4);
	const std::vector<int> &lens = R.lens;
	const int max_len = R.max_len;
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
	std::vector<int> order(n_reads);
	c2a_launch_order(n_reads, nseeds.data(), order.data());

	hipStream_t st = 0;
	const size_t n4 = (size_t)n_reads * 4, tmp_bytes = reg_pack_tmp_bytes(n_reads);
	DevArr<uint8_t> d_seq(R.flat.size(), R.flat.data());
	DevArr<int64_t> d_off((size_t)(n_reads + 1) * 8, R.slot.data());
	DevArr<int> d_len(n4, lens.data()), d_cbeg(n4, chain_beg.data()), d_ccnt(n4, chain_cnt.data()), d_rbeg(n4, reg_beg.data());
	DevArr<int> d_nregs(n4 + 4), d_tab(tab.size() * 4, tab.data()), d_order(n4, order.data()), d_reg_pos(n4 + 4);
	DevArr<DevChain> d_ch(hch.size() * sizeof(DevChain), hch.data());
	DevArr<DevSeed> d_sd(hsd.size() * sizeof(DevSeed), hsd.data());
	DevArr<unsigned int> d_srt(hsrt.size() * 4, hsrt.data());
	DevArr<DevReg> d_regs(hsd.size() * sizeof(DevReg)), d_packed(hsd.size() * sizeof(DevReg));
	DevArr<unsigned long long> d_stat(C2A_STAT_SLOTS * 64);
	DevArr<void> d_tmp(tmp_bytes);
	d_stat.zero();
	{
		C2aGroupBufs B;
		C2aJob J;
		J.n_reads = n_reads; J.max_len = max_len; J.d_seq = d_seq; J.d_off = d_off; J.d_len = d_len;
		J.d_chain_beg = d_cbeg; J.d_chain_cnt = d_ccnt; J.d_reg_beg = d_rbeg; J.d_order = d_order;
		J.d_chains = d_ch; J.d_seeds = d_sd; J.d_srt = d_srt; J.d_tab = d_tab; J.tab_stride = TS; J.d_pac = (const uint8_t *)dev_index().d_pac;
		J.units = c2a_prepare_units(st, B, heavy_t, n_reads, chain_cnt.data(), (size_t)std::max<int64_t>(n_chain_slots, 1), d_cbeg, d_rbeg, d_ch, d_nregs);
		J.d_regs = d_regs; J.d_nregs = d_nregs; J.d_stat = d_stat; J.d_reg_pos = d_reg_pos; J.d_packed = d_packed; J.d_tmp = d_tmp; J.tmp_bytes = tmp_bytes;
		queue_c2a(st, opt, l_pac, early, J);
		HIP_OK(hipStreamSynchronize(st));
		HIP_OK(hipGetLastError());
		if (n_units) *n_units = J.units.max_units;
		B.release();
	}
	std::vector<int> nregs(n_reads), reg_pos(n_reads + 1);
	std::vector<unsigned long long> stat(C2A_STAT_SLOTS * 8);
	d_nregs.download(nregs.data(), n4);
	d_reg_pos.download(reg_pos.data(), n4 + 4);
	d_stat.download(stat.data(), C2A_STAT_SLOTS * 64);
	std::vector<DevReg> regs(std::max(reg_pos[n_reads], 1));
	d_packed.download((void *)regs.data(), (size_t)reg_pos[n_reads] * sizeof(DevReg));
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
// instantiation.  out_hdr5 per request: score, NM, n_cigar, md_len, flags.  read[i] == -1 is an unused slot of the request array, as
// the pipeline leaves them (aln_classify_kernel); the headers are filled with -1 before the launch, so such a slot, and any live
// request that no instantiation answered, comes back with flags = -1.
static std::atomic<uint64_t> g_aln_counts[4];   // of the last call: lengths of the three request lists, pool bytes handed out
extern "C" void mi355x_global_batch_counts(uint64_t out[4])
{
	for (int k = 0; k < 4; ++k) out[k] = g_aln_counts[k].load();
}
extern "C" int mi355x_global_batch(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, int n_reads, const uint8_t *reads,
                                   const int64_t *off, int n_req, const int64_t *rb, const int64_t *re, const int *read,
                                   const int *qb, const int *qe, const int *w, const int *truesc, int which,
                                   int *out_hdr5, uint32_t *cigar_out, int cigar_cap, char *md_out, int md_cap, double *kernel_ms)
{
	require_any_device();
	if (n_req <= 0) return 0;
	hipStream_t st = 0;
	const PackedReads R = pack_reads(n_reads, reads, off, 4);
	const int max_len = R.max_len;
	std::vector<AlnReq> rq(n_req);
	for (int i = 0; i < n_req; ++i) {
		if (read[i] != -1 && (read[i] < 0 || read[i] >= n_reads || rb[i] < 0 || re[i] > 2 * l_pac)) die("mi355x_global_batch: bad request %d", i);
		rq[i].rb = rb[i]; rq[i].re = re[i]; rq[i].read = read[i]; rq[i].qb = qb[i]; rq[i].qe = qe[i]; rq[i].w2 = w[i]; rq[i].truesc = truesc[i];
		rq[i].pad = 0;
	}
	std::vector<int> gaptab;
	cigar_gap_table(opt, max_len, gaptab);
	// (not aln_pool_bytes: a test may ask for nothing but long gapped alignments, whose CIGAR and MD outgrow the pipeline's 96-byte average)
	const size_t pool_bytes = (size_t)n_req * (4 * 96 + 768) + ((size_t)48 << 20);
	DevArr<uint8_t> d_seq(R.flat.size(), R.flat.data()), d_pac(l_pac / 4 + 16, pac, l_pac / 4 + 1), d_pool(pool_bytes);
	DevArr<int64_t> d_off((size_t)(n_reads + 1) * 8, R.slot.data());
	DevArr<AlnReq> d_req((size_t)n_req * sizeof(AlnReq), rq.data());
	DevArr<AlnHdr> d_hdr((size_t)n_req * sizeof(AlnHdr));
	DevArr<int> d_gap(gaptab.size() * 4, gaptab.data()), d_lists((size_t)n_req * 3 * 4);
	DevArr<unsigned long long> d_cnt(256);
	d_cnt.zero();
	d_hdr.fill(0xff);   // flags = -1: written by nobody
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
	d_hdr.download((void *)hdr.data(), (size_t)n_req * sizeof(AlnHdr));
	d_pool.download(pool.data(), pool_bytes);
	{
		unsigned long long cnt[ALN_CNT + 3];
		d_cnt.download(cnt, sizeof cnt);
		for (int k = 0; k < 3; ++k) g_aln_counts[k] = cnt[ALN_CNT + k];
		g_aln_counts[3] = cnt[0];
	}
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
                     unsigned long long *cursor, void *hdr_out, const uint8_t *n_lines = nullptr)
{
	require_any_device();
	if (n_units <= 0) return 0;
	hipStream_t st = 0;
	const int n = ends * n_units, n_req = req_base[n_units];
	const int64_t l_pac = bns->l_pac;
	// n_lines given (one count per read): desc_ holds SE_LINES_CAP line descriptors per read for sam_lines_kernel (ends = 2: its paired
	// instantiation, every pair a unit), and the chunk-wide descriptors say "not the device's", as in the pipeline
	SamDesc not_mine;
	memset(&not_mine, 0, sizeof not_mine);
	not_mine.req = -1;
	const std::vector<SamDesc> none(n_lines ? (size_t)n : 0, not_mine);
	const SamDesc *ldesc = n_lines ? (const SamDesc *)desc_ : nullptr;
	const SamDesc *desc = n_lines ? none.data() : (const SamDesc *)desc_;
	const AlnReq *reqs = (const AlnReq *)reqs_;
	for (int i = 0; i < n; ++i)
		if ((int)(off[i + 1] - off[i]) <= 0 || name_off[i + 1] < name_off[i]) die("%s: bad read %d", who, i);
	const PackedReads R = pack_reads(n, reads, off, 4);
	const std::vector<int> &lens = R.lens;
	const int max_len = R.max_len;
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
	for (int r = 0; n_lines && r < n; ++r) {   // (ends = 2: n_lines by read, 0 = the unaligned record; the lines of pair k count from req_base[k])
		const int k = r / ends;
		if (n_lines[r] == 0) continue;
		if ((ends == 1 && n_lines[r] < 2) || n_lines[r] > SE_LINES_CAP) die("%s: read %d with %d lines", who, r, (int)n_lines[r]);
		for (int j = 0; j < n_lines[r]; ++j) {
			const SamDesc &d = ldesc[(size_t)r * SE_LINES_CAP + j];
			const int q = req_base[k] + d.req;
			if (d.req < 0 || q >= req_base[k + 1] || d.rid < 0 || d.rid >= bns->n_seqs || reqs[q].read != r) die("%s: bad descriptor of line %d of read %d", who, j, r);
			if (d.rb < 0 || d.re > 2 * l_pac || d.rb >= d.re || d.qb < 0 || d.qe > lens[r] || d.qb > d.qe) die("%s: bad region of line %d of read %d", who, j, r);
			for (int x = 1; x <= (d.flag >> SAM_XA_SHIFT & SAM_XA_MASK); ++x)
				if (q + x >= req_base[k + 1] || reqs[q + x].read != r || reqs[q + x].pad < 0 || reqs[q + x].pad >= bns->n_seqs || reqs[q + x].rb >= reqs[q + x].re)
					die("%s: bad XA request %d of line %d of read %d", who, x, j, r);
		}
	}
	for (int q = 0; q < n_req; ++q) {
		const AlnReq &r = reqs[q];
		if (r.read < 0) continue;
		if (r.read >= n || r.rb < 0 || r.re > 2 * l_pac || r.rb > r.re || r.qb < 0 || r.qb > r.qe || r.qe > lens[r.read]) die("%s: bad request %d", who, q);
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
	const size_t req_slots = (size_t)std::max(n_req, 1), pool_bytes = aln_pool_bytes(req_slots), n_names = (size_t)name_off[n];
	DevArr<uint8_t> d_seq(R.flat.size(), R.flat.data()), d_qual, d_pac(l_pac / 4 + 16, pac, l_pac / 4 + 1), d_pool(pool_bytes);
	if (quals) d_qual = DevArr<uint8_t>(R.flat.size(), pack_reads(n, quals, off, 0).flat.data());   // the qualities in the reads' slots
	DevArr<int64_t> d_off((size_t)(n + 1) * 8, R.slot.data()), d_ao(ann_off.size() * 8, ann_off.data());
	DevArr<int> d_len((size_t)n * 4, lens.data()), d_gap(gaptab.size() * 4, gaptab.data()), d_lists(req_slots * 3 * 4);
	DevArr<AlnReq> d_req(req_slots * sizeof(AlnReq), reqs, (size_t)n_req * sizeof(AlnReq));
	DevArr<AlnHdr> d_hdr(req_slots * sizeof(AlnHdr));
	DevArr<unsigned long long> d_cnt(256), d_used(64), d_ooff((size_t)n * 8);
	DevArr<uint8_t> d_names(n_names + 64, names, n_names), d_arena(arena_bytes + SAM_GUARD);
	DevArr<char> d_cn(cn.size() + 64, cn.data(), cn.size());
	DevArr<int> d_noff((size_t)(n + 1) * 4, name_off), d_cno(cno.size() * 4, cno.data()), d_base((size_t)(n_units + 1) * 4), d_olen((size_t)n * 4);
	DevArr<SamDesc> d_desc((size_t)n * sizeof(SamDesc), desc);
	d_hdr.zero();
	d_arena.fill(SAM_GUARD_BYTE);
	d_ooff.zero();
	d_olen.fill(0xff);
	ChunkDev D;
	D.d_seq = d_seq; D.d_off = d_off; D.d_len = d_len; D.max_len = max_len; D.d_pac = d_pac; D.d_gap = d_gap;
	D.d_qual = d_qual; D.d_names = d_names; D.d_noff = d_noff; D.d_ann_off = d_ao; D.d_ann_names = d_cn; D.d_ann_noff = d_cno;
	DevArr<uint8_t> d_ml;
	DevArr<SamDesc> d_md;
	AlnSamJob J;
	if (n_lines) {
		d_ml = DevArr<uint8_t>((size_t)n + 64, n_lines, (size_t)n);
		d_md = DevArr<SamDesc>((size_t)n * SE_LINES_CAP * sizeof(SamDesc), ldesc);
		J.n_multi = n_units; J.d_mlines = d_ml; J.d_mdesc = d_md; J.d_mbase = d_base;   // (every read a unit; its request base is the job's own)
	}
	J.n_req = n_req; J.d_req = d_req; J.d_hdr = d_hdr; J.d_pool = d_pool; J.pool_bytes = pool_bytes; J.d_cnt = d_cnt; J.d_lists = d_lists;
	J.ends = ends; J.n_reads = n; J.d_desc = d_desc; J.h_base = req_base; J.d_base = d_base;
	J.d_arena = d_arena; J.arena_bytes = arena_bytes; J.d_used = d_used; J.d_ooff = d_ooff; J.d_olen = d_olen; J.grid_blocks = grid_blocks;
	queue_aln_sam(st, opt, l_pac, D, sp, J);
	HIP_OK(hipStreamSynchronize(st));
	HIP_OK(hipGetLastError());
	d_olen.download(out_len, (size_t)n * 4);
	d_ooff.download(out_off, (size_t)n * 8);
	d_arena.download(arena_out, arena_bytes + SAM_GUARD);
	d_used.download(cursor, 8);
	if (n_req) d_hdr.download(hdr_out, (size_t)n_req * sizeof(AlnHdr));
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

// The twin for single-end reads of several lines (sam_lines_kernel.hip behind aln_kernel and an idle sam_emit_kernel<false>, as the pipeline
// queues them): n_lines[r] = 2 .. mi355x_se_lines_cap() lines of read r (0: not a read of the device's, out_len = -2), desc_ = their
// descriptors by (r, line) as mi355x_se_wave_lines_batch returns them (req relative to req_base[r]; requests laid out as [line 0, its
// XA entries, line 1, ...]).  out_len[r] = bytes of all lines of the read, back to back at out_off[r]; -1: the host's read.
extern "C" int mi355x_sam_se_lines_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_reads, const uint8_t *reads, const int64_t *off,
                                         const uint8_t *quals, const char *names, const int *name_off, const uint8_t *n_lines, const void *desc_,
                                         const void *reqs_, const int *req_base, size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off,
                                         uint8_t *arena_out, unsigned long long *cursor, void *hdr_out)
{
	if (!n_lines) die("mi355x_sam_se_lines_batch: no line counts");
	return sam_batch("mi355x_sam_se_lines_batch", 1, opt, bns, pac, n_reads, reads, off, quals, names, name_off, desc_, reqs_, req_base, arena_bytes, grid_blocks,
	                 out_len, out_off, arena_out, cursor, hdr_out, n_lines);
}
// The twin for pairs reported end by end (the paired instantiation of sam_lines_kernel behind aln_kernel and an idle sam_emit_kernel<true>):
// every pair is a unit; n_lines[2k + e] = 0 .. mi355x_se_lines_cap() lines of end e (0: the unaligned record), desc_ = the descriptors by
// (read, line) as mi355x_pair_wave_lines_batch returns them (req relative to req_base[k]; requests laid out as [end 0: line 0, its XA
// entries, line 1, ...; end 1: ...], reqs.read = 2k + e).  out_len[r] = bytes of all lines of read r; -1: the host's pair, both reads.
extern "C" int mi355x_sam_pe_lines_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_pairs, const uint8_t *reads, const int64_t *off,
                                         const uint8_t *quals, const char *names, const int *name_off, const uint8_t *n_lines, const void *desc_,
                                         const void *reqs_, const int *req_base, size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off,
                                         uint8_t *arena_out, unsigned long long *cursor, void *hdr_out)
{
	if (!n_lines) die("mi355x_sam_pe_lines_batch: no line counts");
	return sam_batch("mi355x_sam_pe_lines_batch", 2, opt, bns, pac, n_pairs, reads, off, quals, names, name_off, desc_, reqs_, req_base, arena_bytes, grid_blocks,
	                 out_len, out_off, arena_out, cursor, hdr_out, n_lines);
}
extern "C" int mi355x_sam_lines_row(void) { return sam_lines_row(); }
extern "C" int mi355x_sam_lines_sa_stage(void) { return sam_lines_sa_stage(); }

// Stage-level entry point of the seed enumeration between SMEM and SA lookup (tests): seed_prep_kernel, the pipeline's prefix sum over
// the seed counts, seed_enum_kernel, on chosen intervals (read r: n_intv[r] records of (x0, x1, size, info) from intv[r * cap * 4], in any
// order; n_intv[r] > cap: the kernels look at the first cap).  intv comes back sorted by info; rows / qbeg_len: per seed the BWT row
// and (qbeg, len), read r from seed_off[r].  Returns the number of seeds, or -1 - that number when it exceeds seed_cap (then only
// n_seeds, l_rep and seed_off are valid).
extern "C" int64_t mi355x_seed_batch(int n_reads, int cap, int max_occ, uint64_t *intv, const int *n_intv, int *n_seeds, int *l_rep,
                                     int64_t *seed_off, uint64_t *rows, int32_t *qbeg_len, int64_t seed_cap)
{
	require_any_device();
	if (n_reads <= 0) return 0;
	if (cap <= 0 || max_occ <= 0) die("mi355x_seed_batch: cap and max_occ must be positive");
	hipStream_t st = 0;
	const size_t n_words = (size_t)n_reads * cap * 4, n4 = (size_t)n_reads * 4;
	DevArr<uint64_t> d_intv(n_words * 8, intv);
	DevArr<int> d_nintv(n4, n_intv), d_ns(n4), d_lrep(n4);
	DevArr<int64_t> d_so((size_t)(n_reads + 1) * 8);
	launch_seed_prep(st, n_reads, cap, d_intv, d_nintv, max_occ, d_ns, d_lrep);
	HIP_OK(hipStreamSynchronize(st));
	HIP_OK(hipGetLastError());
	d_ns.download(n_seeds, n4);
	d_lrep.download(l_rep, n4);
	d_intv.download(intv, n_words * 8);
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
		DevArr<uint64_t> d_rows((size_t)room * 8);
		DevArr<int32_t> d_qbl((size_t)room * 8);
		d_rows.fill(0xff);
		d_qbl.fill(0xff);
		HIP_OK(hipMemcpy(d_so, seed_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice));
		launch_seed_enum(st, n_reads, cap, d_intv, d_nintv, max_occ, d_so, d_rows, d_qbl);
		HIP_OK(hipStreamSynchronize(st));
		HIP_OK(hipGetLastError());
		d_rows.download(rows, (size_t)S * 8);
		d_qbl.download(qbeg_len, (size_t)S * 8);
	}
	return fits ? S : -1 - S;
}
