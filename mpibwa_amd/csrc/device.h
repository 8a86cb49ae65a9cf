// device.h — host-visible interface of the HIP side (device.hip, stage_entries.hip and the kernel files)
#ifndef MBW_DEVICE_H
#define MBW_DEVICE_H
#include "internal.h"
#include <mutex>
#include <vector>

namespace mbw {

// FM-index constants passed by value to kernels.  The occ blocks keep the
// reference's 64-byte geometry (4 x u64 running counts + 8 x u32 packed
// bases per 128 BWT symbols, src/bwt.h:72-73) but live in a 256-B aligned
// HBM buffer so that one quad (4 lanes x 16 B) fetches a block in one
// coalesced 64-B request.
struct FmDev {
	const void *blk;        // n_blk x 64 B
	const void *occ32;      // device-only occ table of the seeding kernel (fm_kernels.hip): per 32 rows of the BWT with sentinel and per base 16 B {count, count of greater symbols, plane, plane of greater symbols}
	const void *occ_sb;     // its superblock records: absolute counts before every 2^31 rows
	const uint64_t *sa;     // sampled SA, sa[0] = -1
	const uint64_t *sa_full; // optional: SA value of EVERY row (seq_len+1 entries), expanded in HBM at upload; null if absent
	uint64_t primary, seq_len;
	uint64_t L2[5];
	int sa_shift;           // log2(sa_intv)
	// optional jump table of the third seeding pass: bi-interval after the first p3_k forward extensions of every
	// (p3_k + 1)-mer, 32 B per entry {x0, x1, x2, blocks touched}; null if absent
	const void *p3tab;
	int p3_k;
	// optional k-mer tables of the seeding kernel (fm_kernels.hip: kmt_build_kernel): the bi-interval of EVERY string of
	// 1 .. kmt_k bases, 16 B per entry in the interval list's packing, the table of length L at entry (4^L - 4) / 3;
	// an extension whose result is that short is one independent 16-byte load instead of two dependent occ fetches
	const void *kmt;
	int kmt_k;
};

struct DevIndex {
	int device = -1;
	bool ready = false;
	FmDev fm{};
	void *d_blk = nullptr; size_t blk_bytes = 0;
	void *d_occ32 = nullptr; size_t occ32_bytes = 0;
	void *d_sa = nullptr;  size_t sa_bytes = 0;
	void *d_pac = nullptr; size_t pac_bytes = 0;
	void *d_sa_full = nullptr; size_t sa_full_bytes = 0; double sa_expand_ms = 0;
	void *d_p3tab = nullptr;
	void *d_kmt = nullptr; size_t kmt_bytes = 0;
	int64_t l_pac = 0;
	// what is resident, as the caller's host-side index describes itself (compared on every mem_process_seqs call)
	uint64_t id_primary = 0, id_seq_len = 0, id_L2[5] = {0, 0, 0, 0, 0};
	int id_n_seqs = 0;
	uint64_t id_hash = 0;   // of the contig table (offsets, lengths, names) and the first occ block
};
DevIndex &dev_index();
// true when (bwt, bns) describe the index that is resident; message = what differs
bool index_matches(const bwt_t *bwt, const bntseq_t *bns, const char **what);
// calls of mem_process_seqs currently inside the library (pipeline.hip); index upload / release need it to be 0
int calls_in_flight();
void expect_calls_in_flight(int n);   // pipeline.hip: how many calls the caller says it keeps in flight (mi355x_prewarm)
// serialises "is the index resident / the right one, then count the call in" (mem_process_seqs) against upload and release
std::recursive_mutex &index_mutex();
void note_buffer_growth(size_t from, size_t to, const char *kind);   // counted by mi355x_buffer_growths()

// SMEM seeding parameters (subset of mem_opt_t used by mem_collect_intv)
struct SmemParams {
	int min_seed_len, split_len, split_width, max_mem_intv;
};

// ---- device buffers reused across calls ----
struct DevBuf;
// A DevBuf that is constructed while an owner list is open (pipeline.h: the work buffers of a call context) enters it, so that
// the context's buffers can be given back as a whole: when the index is released, or when another call's buffer does not fit.
extern std::vector<DevBuf *> *g_devbuf_owner;
struct DevBuf {
	void *p = nullptr; size_t cap = 0;
	DevBuf() { if (g_devbuf_owner) g_devbuf_owner->push_back(this); }
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	// grow-only hipMalloc.  A buffer that does not fit asks the pipeline to make room (device_memory_pressure: the buffers of idle
	// call contexts are given back; with other calls in flight the caller waits for one of them to end and fewer calls are admitted
	// from then on) and only a lone call whose buffer still does not fit ends the process.
	void *ensure(size_t bytes);
	void release();
};
// grow-only page-locked host buffer: staging for the bulk H2D / D2H copies (full PCIe rate, no per-chunk page faults)
struct PinBuf {
	void *p = nullptr; size_t cap = 0;
	void *ensure(size_t bytes);
	void release();
};
// pipeline.hip: called when a device allocation has failed; true = something was freed or a call has ended: try again
bool device_memory_pressure(size_t wanted);
void release_idle_work_buffers();   // all call contexts that are not inside a call (mi355x_finalize)

// Launchers (all asynchronous on `stream`; kernel time measured by the caller with HIP events)
// SMEM seeding: two launches on the stream — the third pass (smem_kernels.hip, a read per lane) first, then passes 1-2
// (fm_kernels.hip, a read per quad), which append to its output.
// d_off[r] must be a multiple of 16 (reads padded to 16-byte slots); d_len[r] is the true length
void launch_smem(void *stream, const FmDev &fm, const SmemParams &sp, int n_reads, const uint8_t *d_seq,
                 const int64_t *d_off, const int *d_len, int cap, uint64_t *d_out, int *d_nout, int max_len,
                 unsigned long long *d_counters /* zeroed; [1]=blocks, [2]=overflow on return */,
                 void *d_scratch, size_t scratch_bytes_per_quad, int n_quads,
                 bool count_blocks /* counters[1] += the reference's occ blocks of passes 1-2 (the third pass always counts) */);
size_t occ32_bytes(uint64_t seq_len);
size_t kmt_bytes(int k);                                         // all tables of lengths 1 .. k
void launch_kmt_build(void *stream, const FmDev &fm, int k, void *d_tab);   // needs fm.occ32; level by level on the stream
void launch_occ32_build(void *stream, FmDev &fm, void *d_buf);   // from fm.blk (bwa format), after upload / broadcast; sets fm.occ32 / fm.occ_sb
int  smem_grid_quads(int max_len, size_t *scratch_per_quad);
void launch_smem_p3(void *stream, const FmDev &fm, const SmemParams &sp, int n_reads, const uint8_t *d_seq, const int64_t *d_off,
                    const int *d_len, int cap, uint64_t *d_out, int *d_nout, unsigned long long *d_counters);
// fills tab (4^(k+1) entries of 32 B) with the state of bwt_seed_strategy1 after k forward extensions of every (k+1)-mer
void launch_p3_build(void *stream, const FmDev &fm, int k, void *d_tab);

void launch_sa(void *stream, const FmDev &fm, int n, const uint64_t *d_k, uint64_t *d_out,
               unsigned long long *d_counters /* [0]=next task, [1]=steps */);
// dense-SA path: one 8-byte load per lookup from FmDev::sa_full
void launch_sa_dense(void *stream, const FmDev &fm, int n, const uint64_t *d_k, uint64_t *d_out);
// fill `full` (seq_len+1 entries) from the sampled SA by walking LF once over the whole text (seq_len steps in total)
void launch_sa_expand(void *stream, const FmDev &fm, uint64_t *full, unsigned long long *d_counters);

struct ExtParams {
	int8_t mat[25];
	int o_del, e_del, o_ins, e_ins, zdrop;
};
ExtParams ext_params(const mem_opt_t *opt);
void launch_extend(void *stream, const ExtParams &ep, int n, const uint8_t *d_q, const int64_t *d_qoff,
                   const uint8_t *d_t, const int64_t *d_toff, const int *d_w, const int *d_h0, const int *d_eb,
                   int *d_out6, unsigned long long *d_cells, int max_qlen);
// per job: early != 0 = the row loop that stops as soon as nothing the caller of c2a_kernel reads can change, with the job's clipping
// penalty; d_cells: one count per job
void launch_extend2(void *stream, const ExtParams &ep, int n, const uint8_t *d_q, const int64_t *d_qoff,
                    const uint8_t *d_t, const int64_t *d_toff, const int *d_w, const int *d_h0, const int *d_early, const int *d_clip,
                    int *d_out6, unsigned long long *d_cells, int max_qlen);

// ---- chain -> region kernel (c2a_kernel.hip) ----
struct DevSeed { int64_t rbeg; int32_t qbeg, len; };           // 16 B
struct DevChain {
	int64_t far_beg, far_end;    // bounds of the chain's contig on the chain's strand (doubled coordinate)
	int32_t seed_beg, n_seeds;   // into the flat seed / order arrays
	int32_t rid;
	float frac_rep;
	int64_t rmax0, rmax1;        // the reference window of mem_chain2aln (src/bwamem.c:642-661), already clamped
};
struct DevReg {                  // the fields of mem_alnreg_t that mem_chain2aln fills (src/bwamem.c:708-783)
	int64_t rb, re;
	int32_t qb, qe, rid, score, truesc, w, seedcov, seedlen0;
	float frac_rep;
	int32_t pad;
};
struct C2aParams {
	int64_t l_pac;
	int a, w, pen_clip5, pen_clip3;
	int early;    // 1: row loops end as soon as no output the kernel reads can change (wave_ext.cuh); 0: the reference's rows; 2: both, differences counted
};
// Reads with more than `heavy_t` chains are not walked by one wavefront: their chains are split into independent groups
// (c2a_groups.hip) and every group is a unit of its own.  max_units = 0: no such reads in the launch.
struct C2aUnits {
	int max_units = 0, heavy_t = 0;
	const unsigned int *n_units = nullptr;   // units that exist (<= max_units)
	const int *ustart = nullptr;             // unit u: chains clist[ustart[u] .. ustart[u + 1])
	const int *unit_rd = nullptr, *unit_av = nullptr;   // its read; first region slot of the unit
	const int *clist = nullptr;
	int *c_rabs = nullptr, *c_rcnt = nullptr;           // per chain (same numbering as the chain array): where its regions are, how many
};
// what the units of a launch need: launch_c2a_groups' inputs, outputs and scratch, the per-chain region places, the unit count read back
struct C2aGroupBufs {
	PinBuf h_heavy, h_hoff, h_nunits;
	DevBuf heavy, hoff, scratch, clist, ustart, unit_rd, unit_av, nunits, c_rabs, c_rcnt;
	void release()   // every member above
	{
		for (PinBuf *b : {&h_heavy, &h_hoff, &h_nunits}) b->release();
		for (DevBuf *b : {&heavy, &hoff, &scratch, &clist, &ustart, &unit_rd, &unit_av, &nunits, &c_rabs, &c_rcnt}) b->release();
	}
};
// The units of the reads with more than heavy_t chains (chain_cnt: host copy of d_chain_cnt; n_chain_slots: size of the chain array):
// launch_c2a_groups on `stream`, then one round trip for the number of units, which sizes launch_c2a's grid.  With units, d_nregs
// (n + 1 entries) is zeroed on `stream` behind them.  max_units = 0: heavy_t is 0 or no read has that many chains.  wait: how to wait
// for the stream (null: hipStreamSynchronize).
C2aUnits c2a_prepare_units(void *stream, C2aGroupBufs &B, int heavy_t, int n, const int *chain_cnt, size_t n_chain_slots, const int *d_chain_beg,
                           const int *d_reg_beg, const DevChain *d_chains, int *d_nregs, void (*wait)(void *stream) = nullptr);
// c2a_kernel's launch order: the reads by decreasing number of seeds (counting sort), the long-running ones first
void c2a_launch_order(int n, const int *nseeds, int *order);
// the length tables of c2a_kernel (rows gap, bound5, bound3, ceil95, thr10) and chain_kernel (row 5: mem_flt_chained_seeds is a no-op),
// max_len + 2 entries per row: the reference's floating-point decisions resolved per length
void c2a_length_tables(const mem_opt_t *opt, int max_len, std::vector<int> &tab);
void c2a_params(const mem_opt_t *opt, int64_t l_pac, int early, C2aParams &cp, ExtParams &ep);
size_t c2a_groups_scratch_bytes(int n_el);
void launch_c2a_groups(void *stream, int n_el, int n_heavy, const int *d_hoff, const int *d_heavy, const int *d_chain_beg, const int *d_reg_beg,
                       const DevChain *d_chains, void *d_scratch, int *d_clist, int *d_ustart, int *d_unit_rd, int *d_unit_av, unsigned int *d_n_units);
// counters of c2a_kernel: C2A_STAT_SLOTS lines of 8 u64 (zeroed by the caller, summed by the caller): [0] DP cells computed, [1] extensions,
// [2] extensions answered without DP, [3] (early = 2) extensions whose used outputs differ
#define C2A_STAT_SLOTS 256
void launch_c2a(void *stream, const C2aParams &P, const ExtParams &ep, int n_reads, const uint8_t *d_seq, const int64_t *d_off,
                const int *d_len, const int *d_chain_beg, const int *d_chain_cnt, const DevChain *d_chains, const DevSeed *d_seeds, unsigned int *d_srt,
                const int *d_reg_beg, DevReg *d_regs, int *d_nregs, const int *d_tab, int tab_stride, const uint8_t *d_pac, unsigned long long *d_counters,
                int max_len, const int *d_order = nullptr, const C2aUnits *units = nullptr /* then d_nregs must be zeroed */);

// ---- seeds -> chains -> filtered chains on the device (chain_kernel.hip) ----
struct ChainParams {
	int64_t l_pac;
	int w, max_chain_gap, min_chain_weight, min_seed_len, max_chain_extend;
	float mask_level, drop_ratio;
};
ChainParams chain_params(const mem_opt_t *opt, int64_t l_pac);
// the contig table of the chaining and pairing kernels: ann_off[k] = start of contig k, ann_off[n_seqs] = l_pac; ann_alt[k] = its ALT flag
// (n_seqs + 1 entries each)
void contig_table(const bntseq_t *bns, std::vector<int64_t> &ann_off, std::vector<uint8_t> &ann_alt);
// Per read r: chains / seeds / order are written at index seed_off[r] onwards (a read never keeps more seeds or chains
// than it had seeds); n_chains[r] = number of kept chains, or < 0 when the read needs the host path (more than 4 096 seeds,
// two chains at one position, or long enough for mem_flt_chained_seeds).  d_tab: the length tables of c2a (rows 0 and 5 are read:
// the gap table and "flt is a no-op").  d_scratch: chain_scratch_bytes(n_reads) bytes (lists, counters, the persistent waves' slices).
void launch_chain(void *stream, const ChainParams &P, int n_reads, const int *d_len, const int *d_nseeds, const int *d_lrep,
                  const int64_t *d_seed_off, const uint64_t *d_sa, const int32_t *d_qbl, const int64_t *d_ann_off, const uint8_t *d_ann_alt,
                  int n_seqs, const int *d_tab, int tab_stride, DevChain *d_chains, DevSeed *d_seeds, unsigned int *d_srt, int *d_nchains,
                  void *d_scratch);
size_t chain_scratch_bytes(int n_reads);

size_t reg_pack_tmp_bytes(int n_reads);
void launch_reg_pack(void *stream, int n_reads, const int *d_reg_beg, const int *d_nregs, int *d_reg_pos, const DevReg *d_regs, DevReg *d_packed,
                     void *d_tmp, size_t tmp_bytes, const C2aUnits *units = nullptr, const int *d_chain_beg = nullptr, const int *d_chain_cnt = nullptr);
// One chain -> regions job: c2a_kernel over the chains of n_reads reads, then the prefix sum and pack of their regions, queued on one
// stream.  Phase 1 of the pipeline (phase1.hip: extend) and the stage entry (stage_entries.hip: mi355x_c2a_batch) both queue it through
// queue_c2a(), which allocates nothing: every array is the caller's, sized before (the pipeline calls it while it holds a turn).
struct C2aJob {
	int n_reads = 0, max_len = 0;
	const uint8_t *d_seq = nullptr; const int64_t *d_off = nullptr; const int *d_len = nullptr;   // the reads of the job
	const int *d_chain_beg = nullptr, *d_chain_cnt = nullptr, *d_reg_beg = nullptr, *d_order = nullptr;   // per read; d_order: c2a_launch_order
	const DevChain *d_chains = nullptr; const DevSeed *d_seeds = nullptr; unsigned int *d_srt = nullptr;
	const int *d_tab = nullptr; int tab_stride = 0;   // c2a_length_tables
	const uint8_t *d_pac = nullptr;
	C2aUnits units;                                   // from c2a_prepare_units (a round trip: before the job is queued)
	DevReg *d_regs = nullptr; int *d_nregs = nullptr;  // sparse per-read slots, n_reads + 1 counts
	unsigned long long *d_stat = nullptr;              // C2A_STAT_SLOTS lines, zeroed by the caller
	int *d_reg_pos = nullptr; DevReg *d_packed = nullptr; void *d_tmp = nullptr; size_t tmp_bytes = 0;   // reg_pack: n_reads + 1 places, the packed list, reg_pack_tmp_bytes(n_reads)
};
// on `stream`: [ev_a] c2a_kernel [ev_b], reg_pack.  early: C2aParams::early; ev_a / ev_b: hipEvent_t around the kernel, or null
void queue_c2a(void *stream, const mem_opt_t *opt, int64_t l_pac, int early, const C2aJob &J, void *ev_a = nullptr, void *ev_b = nullptr);

// ---- final global re-alignment on the device (aln_kernel.hip) ----
struct AlnReq {                  // one call of mem_reg2aln's DP loop (src/bwamem.c:1106-1122)
	int64_t rb, re;
	int32_t read, qb, qe, w2, truesc, pad;
};
struct AlnHdr {                  // result header; cigar (n_cigar x u32) and MD (md_len bytes) sit at pool[4 * pool_off]
	int32_t score, NM, n_cigar, md_len;
	uint32_t pool_off;
	int32_t flags;               // 1 = not done on the device (band matrix too large / caps): the host recomputes it
};
struct AlnParams { int64_t l_pac; int a, w; };
#define ALN_CNT 8                // launch_aln's d_counters: [0] pool bytes handed out, [ALN_CNT + k] length of the request list of kind k
void aln_params(const mem_opt_t *opt, int64_t l_pac, AlnParams &ap, ExtParams &ep);
// the result pool of n_req requests: 96 bytes each + room for the partly used last slab of every wave (aln_kernel.hip: ALN_SLAB)
inline size_t aln_pool_bytes(size_t n_req) { return n_req * 96 + ((size_t)48 << 20); }
// max_gap of bwa_gen_cigar2 (src/bwa.c:155-158), a function of l_query only: max_len + 2 entries
void cigar_gap_table(const mem_opt_t *opt, int max_len, std::vector<int> &tab);
size_t aln_lds_per_block(int max_len, int tcap);   // LDS of the full-size CIGAR kernel for reads of up to max_len bases
void launch_aln(void *stream, const AlnParams &P, const ExtParams &ep, int n_req, const AlnReq *d_req, const uint8_t *d_seq,
                const int64_t *d_off, const uint8_t *d_pac, const int *d_gaptab, AlnHdr *d_hdr, uint8_t *d_pool,
                unsigned long long *d_counters, size_t pool_bytes, int max_len, int tcap, int *d_lists /* 3 * n_req ints of scratch */,
                bool wide_only = false /* DP requests skip the narrow-band instantiation (stage tests) */);

// ---- SAM text of confidently paired reads on the device (sam_kernel.hip) ----
struct SamDesc {                 // one output line: the chosen hit of a read as mem_sam_pe's paired branch reports it
	int64_t rb, re;              // region in the doubled coordinate
	int32_t qb, qe;
	int32_t req;                 // its CIGAR request, relative to the first request of the pair; < 0: the line is not the device's
	int32_t rid, flag, mapq, score, sub;   // flag: the SAM flag in bits 0-15; bits 16-19: the number of XA entries of the line, whose
	                                       // requests follow the line's own (AlnReq::pad = the entry's contig)
};
#define SAM_XA_SHIFT 16
#define SAM_XA_MASK 15
struct SamParams {
	int64_t l_pac;
	int has_qual, rg_len;
	char rg[256];                // bwa_rg_id
};
SamParams sam_params(int64_t l_pac, bool has_qual);   // + the read group, bwa_rg_id
// the contig names back to back; name k is names[name_off[k] .. name_off[k + 1])
void contig_names(const bntseq_t *bns, std::vector<char> &names, std::vector<int> &name_off);
size_t sam_arena_bytes(int n_reads, int max_len);   // the arena the pipeline gives n_reads records of reads of up to max_len bases
// One CIGAR-and-SAM job: aln_kernel over n_req requests, then sam_emit_kernel over the records of n_reads reads, queued on one stream.
// The SAM stage (sam_stage.hip: the host's units and the units decided on the device) and the stage entries (stage_entries.hip: sam_batch)
// all queue it through queue_aln_sam().
struct ChunkDev {                // what is resident of the chunk: packed reads, qualities, names, the contig table, the CIGAR gap table
	const uint8_t *d_seq = nullptr; const int64_t *d_off = nullptr; const int *d_len = nullptr; int max_len = 0;
	const uint8_t *d_pac = nullptr; const int *d_gap = nullptr;
	const uint8_t *d_qual = nullptr, *d_names = nullptr; const int *d_noff = nullptr;
	const int64_t *d_ann_off = nullptr; const uint8_t *d_ann_alt = nullptr; const char *d_ann_names = nullptr; const int *d_ann_noff = nullptr;
};
struct AlnSamJob {
	int n_req = 0; const AlnReq *d_req = nullptr; AlnHdr *d_hdr = nullptr; uint8_t *d_pool = nullptr; size_t pool_bytes = 0;
	unsigned long long *d_cnt = nullptr; int *d_lists = nullptr;
	// the records: reads r0 .. r0 + n_reads of the chunk, `ends` of them per unit (2: pairs, 1: single-end reads); n_reads = 0: no SAM launch
	int ends = 2, r0 = 0, n_reads = 0;
	const SamDesc *h_desc = nullptr;   // of the chunk; given: the job's slice is uploaded to d_desc first
	SamDesc *d_desc = nullptr;         // of the chunk
	const int *h_base = nullptr; int *d_base = nullptr;   // first request of every unit (n_reads / ends + 1 entries), uploaded here
	uint8_t *d_arena = nullptr; size_t arena_bytes = 0; unsigned long long *d_used = nullptr, *d_ooff = nullptr; int *d_olen = nullptr;
	int grid_blocks = 0;
	// the reads with several lines (sam_lines_kernel.hip), whose chunk-wide descriptor says "not the device's": n_multi units.  ends = 1:
	// unit u = read d_mlist[u] of the chunk (null: r0 + u) with d_mlines[u] lines, their descriptors at d_mdesc[u * SE_LINES_CAP ..]
	// and its requests from d_mbase[u] in d_req (d_mlines[u] = 0 or d_mbase[u] < 0: not a unit of this job).  All four live on the device
	// already: in the pipeline they are se_wave_kernel's own work list and side arrays.  ends = 2: the units are pairs reported end by
	// end (pair_wave_kernel: PW_DECIDED_LINES) — unit u = pair d_mlist[u] of the chunk (null: r0 / 2 + u), d_mlines[2u + e] lines of end
	// e (0: the unaligned record) with their descriptors at d_mdesc[(2u + e) * SE_LINES_CAP ..]; d_mbase[u] < 0 alone says "not a unit".
	int n_multi = 0; const int *d_mlist = nullptr; const uint8_t *d_mlines = nullptr; const SamDesc *d_mdesc = nullptr; const int *d_mbase = nullptr;
};
// on `stream`: zero the counters, [ev_a] aln_kernel [ev_b] (when there are requests), then descriptors and request bases up, zero the
// arena cursor, sam_emit_kernel, and sam_lines_kernel behind it on the same arena when the job lists reads with several lines.
// ev_a / ev_b: hipEvent_t around the CIGAR kernel, or null
void queue_aln_sam(void *stream, const mem_opt_t *opt, int64_t l_pac, const ChunkDev &D, const SamParams &sp, const AlnSamJob &J,
                   void *ev_a = nullptr, void *ev_b = nullptr);
// d_req_base[pair] = first CIGAR request of the pair in d_hdr; out_len[r] = bytes of the record at arena + out_off[r],
// -1 = the host must format the pair, -2 = not a line of the device.  grid_blocks > 0 caps the number of workgroups (stage tests:
// the grid-stride loop with a few thousand reads); 0 = the launcher's own choice
// d_req: the requests d_hdr answers (read by the lines with XA entries only; may be null when no descriptor has any)
void launch_sam_emit(void *stream, const SamParams &P, int n_reads, const SamDesc *d_desc, const int *d_req_base, const AlnReq *d_req, const AlnHdr *d_hdr,
                     const uint8_t *d_pool, const uint8_t *d_seq, const int64_t *d_off, const int *d_len, const uint8_t *d_qual,
                     const uint8_t *d_names, const int *d_name_off, const int64_t *d_ann_off, const char *d_ann_names, const int *d_ann_name_off,
                     uint8_t *d_arena, size_t arena_bytes, unsigned long long *d_arena_used, unsigned long long *d_out_off, int *d_out_len,
                     int grid_blocks = 0);
// the single-end instantiation: a unit is one read (d_req_base[read]), no mate descriptor, a read is handed back alone
void launch_sam_emit_se(void *stream, const SamParams &P, int n_reads, const SamDesc *d_desc, const int *d_req_base, const AlnReq *d_req, const AlnHdr *d_hdr,
                        const uint8_t *d_pool, const uint8_t *d_seq, const int64_t *d_off, const int *d_len, const uint8_t *d_qual,
                        const uint8_t *d_names, const int *d_name_off, const int64_t *d_ann_off, const char *d_ann_names, const int *d_ann_name_off,
                        uint8_t *d_arena, size_t arena_bytes, unsigned long long *d_arena_used, unsigned long long *d_out_off, int *d_out_len,
                        int grid_blocks = 0);
// ---- SAM text of single-end reads with several lines (sam_lines_kernel.hip), a read per wavefront ----
// Unit u: read rd = d_list ? d_list[u] - r0 : u of d_off / d_len / d_name_off / d_out_off / d_out_len, d_n_lines[u] lines (2 ..
// SE_LINES_CAP) described by d_ldesc[u * SE_LINES_CAP ..] as se_wave_kernel leaves them (device.h: SeLines), its requests from
// d_req_base[u] in d_req / d_hdr; d_n_lines[u] = 0 or d_req_base[u] < 0: not a unit of the job, nothing of it is touched.  out_len[rd] = bytes of all the read's lines, back to back at arena + out_off[rd], or -1: the host's
// read (a declined CIGAR, short fields of a line beyond sam_lines_row() bytes, an SA entry beyond sam_lines_sa_stage() bytes, an XA
// entry beyond XA_STAGE, a full arena).  The arena cursor is the one sam_emit_kernel advanced: not zeroed here.
void launch_sam_lines(void *stream, const SamParams &P, bool softclip, int n_units, const int *d_list, int r0, const uint8_t *d_n_lines, const SamDesc *d_ldesc,
                      const int *d_req_base, const AlnReq *d_req, const AlnHdr *d_hdr, const uint8_t *d_pool, const uint8_t *d_seq, const int64_t *d_off,
                      const int *d_len, const uint8_t *d_qual, const uint8_t *d_names, const int *d_name_off, const int64_t *d_ann_off,
                      const char *d_ann_names, const int *d_ann_name_off, uint8_t *d_arena, size_t arena_bytes, unsigned long long *d_arena_used,
                      unsigned long long *d_out_off, int *d_out_len, int grid_blocks = 0, bool pe = false);
// pe: the paired instantiation: unit u = pair pr = d_list ? d_list[u] : u, whose reads are 2 pr - r0 + e of the arrays above; d_n_lines[2u + e]
// lines of end e (0 .. SE_LINES_CAP; 0: the unaligned record) described by d_ldesc[(2u + e) * SE_LINES_CAP ..] as pair_wave_kernel
// leaves them, the pair's requests from d_req_base[u]; d_req_base[u] < 0: not a unit.  The mate of every line is line 0 of the other
// end, or the unaligned record.  out_len / out_off per read; a pair is handed back whole (both out_len = -1).
int sam_lines_row(void);
int sam_lines_sa_stage(void);

struct MswReq;
struct MswRes;
// ---- pairing decisions of the pairs with one plain hit per end (pair_kernel.hip) ----
#define PR_MAXREG 8               // regions per read the kernel looks at (a read with more is the host's); 4 until round 4
extern "C" int mi355x_pair_maxreg(void);
struct PairParams {
	int64_t l_pac;
	int a, b, pen_unpaired, min_seed_len, w, o_del, e_del, o_ins, e_ins, max_chain_gap, T, max_matesw;
	float mask_level_redun, mask_level, XA_drop_ratio;
	uint64_t id0;             // number of the chunk's first pair (n_processed >> 1): the hash tie-breaks of src/bwamem.c:527, src/bwamem_pair.c:222
	int lnq[64];              // (int)(4.343 * log(n + 1) + .499), src/bwamem.c:972, src/bwamem_pair.c:313 (the pairing kernels read the first 40,
	                          // se_wave_kernel up to sub_n = PW_MAXREG - 1)
	int no_rescue;            // MEM_F_NO_RESCUE or max_matesw <= 0: mem_sam_pe's rescue loop does not run
	int low[4], high[4], failed[4];   // mem_pestat_t per orientation
	int tab_off[4];           // start of each orientation's run in the pair-score table: entry [dist - low]
	int ltab_n;               // entries of the per-length table
	int max_XA_hits;          // min(max_XA_hits, max_XA_hits_alt): more qualifying secondary hits than this and no XA string is written (pair_wave_kernel)
};
// PairParams from the options and the insert-size statistics; false when the kernel cannot take this chunk (a degenerate
// distribution); *n_tab = entries of the pair-score table.  pair_tables fills tab[n_tab + P.ltab_n] (scores, then the per-length table).
bool pair_params(const mem_opt_t *opt, int64_t l_pac, const mem_pestat_t pes[4], int64_t n_processed, int max_len, PairParams &P, size_t *n_tab);
void pair_tables(const mem_opt_t *opt, const mem_pestat_t pes[4], const PairParams &P, size_t n_tab, double *tab);
// per read of a sub-batch: its first PR_MAXREG regions and its number of regions, into chunk-wide arrays (d_first: PR_MAXREG records per read)
void launch_first_reg(void *stream, int n, const int *d_reg_pos, const int *d_nregs, const DevReg *d_packed, DevReg *d_first, int *d_nfirst);
// status codes of pair_simple_kernel: PR_DECIDED, or the test that left the pair to the host (statistics, and which pairs pair_wave_kernel takes)
#define PR_HOST 0                 // not looked at
#define PR_DECIDED 1              // reqs[2k .. 2k+1] and desc[2k .. 2k+1] are what the host's COLLECT pass would have listed
#define PR_HOST_NO_HIT 2          // an end without a hit, or a pair the host did not pass (comment column, unequal names)
#define PR_HOST_MAXREG 3          // more than PR_MAXREG regions on an end, or more candidate pairs than the kernel sorts
#define PR_HOST_PATCH 4           // two hits the host has to try to patch
#define PR_HOST_LENGTH 6          // a hit on an ALT contig or longer than the per-length table
#define PR_HOST_RESCUE 7          // the rescue loop would align something
#define PR_HOST_NO_PAIR 8         // no pair in a proper orientation and distance: the ends are reported independently
#define PR_HOST_SCORE 9           // the best pair scores nothing
#define PR_HOST_SUPP 10           // an end with a second primary hit of at least T: the single-end logic's case
#define PR_HOST_XA 11             // a secondary hit close enough to its primary for an XA entry
// (desc.req = 0 / 1, relative to the pair's first request; the host's pairs: reqs marked read = -1)
void launch_pair_simple(void *stream, const PairParams &P, int n_pairs, const DevReg *d_first, const int *d_nfirst, const uint8_t *d_ok,
                        const int64_t *d_ann_off, const uint8_t *d_ann_alt, const double *d_ptab, const double *d_ltab, uint8_t *d_status,
                        AlnReq *d_reqs, SamDesc *d_desc);

// ---- pairing decisions of the pairs with mate rescue or up to PW_MAXREG hits per end (pair_wave_kernel.hip), a pair per wavefront ----
#define PW_MAXREG 64              // regions per end, going in and while rescued hits are added
extern "C" int mi355x_pair_wave_maxreg(void);
// status codes of pair_wave_kernel: pair_simple_kernel's where the test is the same (PR_DECIDED too: decided, both records plain), and
// four of its own
#define PW_HOST_LENGTH PR_HOST_LENGTH
#define PW_HOST_NO_PAIR PR_HOST_NO_PAIR
#define PW_HOST_SCORE PR_HOST_SCORE
#define PW_HOST_SUPP PR_HOST_SUPP
#define PW_HOST_XA PR_HOST_XA
#define PW_HOST_NO_RESULT 12      // a rescue alignment the replay needs is not on the device (not listed, flagged by msw2_kernel, host only)
#define PW_HOST_FULL 13           // a list past PW_MAXREG
#define PW_HOST_TIE 14            // the outcome depends on the reference's unstable sorts (equal end positions, equal (score, hash))
#define PW_DECIDED_XA 16          // decided, and at least one of the two records carries an XA tag
#define PW_DECIDED_LINES 17       // decided through no_pairing: (src/bwamem_pair.c:371-392): 0 .. SE_LINES_CAP lines per end (SE_DECIDED_LINES' number)
#define PW_XA_CAP 8               // XA entries per record the kernel lists; a call with max_XA_hits beyond it runs without XA on the device
extern "C" int mi355x_pair_wave_xa_cap(void);
struct SeLines;
// tags per (end, candidate hit, orientation): >= 0 the alignment's number in the pair's slice of the mate-rescue requests
#define PW_TAG_NO_WINDOW (-1)     // mem_matesw would align nothing there (src/bwamem_pair.c:150)
#define PW_TAG_HOST (-2)          // not listed (explained by a mate hit before any rescue) or a window msw2_kernel does not take
// work[t]: the pair's number in the chunk (reads 2 work[t], 2 work[t] + 1 of d_len); reqs / desc [2t + e] are written when
// wstatus[t] = PR_DECIDED or PW_DECIDED_XA and left alone otherwise; lists[loff[2t + e] .. loff[2t + e + 1]): end e's regions after mem_sort_dedup_patch;
// mreq / mres[mfirst[t] + tag]; tags[toff[t] ..]: 4 per candidate hit, end 0's candidates first
void launch_pair_wave(void *stream, const PairParams &P, int n_work, const int *d_work, const DevReg *d_lists, const int *d_loff, const int *d_len,
                      const MswReq *d_mreq, const MswRes *d_mres, const unsigned *d_mfirst, const short *d_tags, const int *d_toff,
                      const int64_t *d_ann_off, const double *d_ptab, const double *d_ltab, uint8_t *d_wstatus, AlnReq *d_reqs, SamDesc *d_desc,
                      AlnReq *d_xa_reqs = nullptr, uint8_t *d_xa_cnt = nullptr, const SeLines *lines = nullptr);
// d_xa_reqs given (and max_XA_hits <= PW_XA_CAP): a pair whose chosen hits carry XA entries (src/bwamem_extra.c:98-118) is decided too,
// with status PW_DECIDED_XA: xa_cnt[2t + e] entries of end e, their requests (as mem_reg2aln would ask, pad = the hit's contig) at
// xa_reqs[(2t + e) * PW_XA_CAP ..], desc[2t + e].flag bits 16-19 = the count, desc[2t].req = 0, desc[2t + 1].req = 1 + xa_cnt[2t].
// lines given (the side arrays of SeLines below, by (work item t, end e, line j): slot x = (2t + e) * SE_LINES_CAP + j of desc / reqs /
// xa_cnt, the XA requests at xa_reqs[x * PW_XA_CAP ..], n_lines[2t + e]): a pair that mem_sam_pe reports end by end through no_pairing:
// (src/bwamem_pair.c:371-392) with at most SE_LINES_CAP lines per end gets PW_DECIDED_LINES instead of PW_HOST_NO_PAIR / _SCORE / _SUPP.
// n_lines = 0: the end's record is the unaligned one, without descriptor or request.  desc.flag = 0x40 << e | 1 (| 2: the top hits make
// a proper pair, :382-387) | supp_flag behind the first line | the XA count in bits 16-19; desc.req counts from the pair's first
// request, laid out as [end 0: line 0, its XA entries, line 1, ...; end 1: ...]; reqs.read = 2 work[t] + e.  reqs / desc / xa_cnt
// [2t + e] of the launch are not written for such a pair.  lines->xa_reqs = nullptr (or max_XA_hits > PW_XA_CAP): a line with 1 ..
// max_XA_hits XA entries gives PW_HOST_XA.  Without the arrays nothing changes.
// the decided pairs' records into the chunk-wide arrays (reqs / desc [2 work[t] + e]); clear_n > 0: reads clear_r0 .. + clear_n are
// marked "not the device's" first (the arrays then describe the wave's pairs alone)
void launch_pair_wave_scatter(void *stream, int n_work, const int *d_work, const uint8_t *d_wstatus, const AlnReq *d_w_reqs, const SamDesc *d_w_desc,
                              AlnReq *d_reqs, SamDesc *d_desc, int clear_r0, int clear_n);

// ---- decisions of the single-end reads that end in one record (se_kernel.hip) ----
// status codes of se_simple_kernel (the numbers of pair_simple_kernel's codes where the test is the same)
#define SE_HOST 0                 // not looked at
#define SE_DECIDED 1              // reqs[i] and desc[i] are what the host's COLLECT pass would have listed (desc.req = 0, or -3: the unmapped record)
#define SE_HOST_COMMENT 2         // the read carries a comment column (-C)
#define SE_HOST_MAXREG 3          // more than PR_MAXREG regions
#define SE_HOST_PATCH 4           // two regions mem_patch_reg would align across
#define SE_HOST_LENGTH 5          // a region longer than the per-length table
#define SE_HOST_ALT 6             // a region on an ALT contig
#define SE_HOST_SUPP 10           // a second primary region of at least T: supplementary line, SA tags
#define SE_HOST_XA 11             // a secondary region within XA_drop_ratio of its primary: XA tag
// PairParams for a single-end call: the options, id0 = n_processed (the hash tie-breaks of src/bwamem.c:527), every orientation
// failed and an empty pair-score table; pair_tables(opt, the same pes, P, 0, tab) then fills the per-length table alone (P.ltab_n entries)
void se_params(const mem_opt_t *opt, int64_t l_pac, int64_t n_processed, int max_len, PairParams &P, mem_pestat_t pes[4]);
// d_first / d_nfirst as launch_first_reg leaves them; d_ok[i] = 0: the host's read whatever its regions; reqs and desc: one record per read
void launch_se_simple(void *stream, const PairParams &P, int n_reads, const DevReg *d_first, const int *d_nfirst, const uint8_t *d_ok,
                      const uint8_t *d_ann_alt, const double *d_ltab, uint8_t *d_status, AlnReq *d_reqs, SamDesc *d_desc);

// ---- decisions of the single-end reads with up to PW_MAXREG regions or an XA tag (se_wave_kernel.hip), a read per wavefront ----
// status codes of se_wave_kernel: se_simple_kernel's where the test is the same (5 length, 6 ALT, 10 second primary hit, 11 XA entries
// without room for them), pair_wave_kernel's numbers for the three of its own
#define SE_HOST_FULL 13           // a list past PW_MAXREG
#define SE_HOST_TIE 14            // two hits equal under (score, hash): the reference's unstable sort decides
#define SE_DECIDED_XA 16          // decided, and the record carries an XA tag (SE_DECIDED: the record is plain)
static_assert(PW_MAXREG <= 64, "PairParams::lnq holds sub_n up to PW_MAXREG - 1");
// work[t]: the read's number in the chunk (id = P.id0 + work[t]); lists[loff[t] .. loff[t + 1]): its regions after mem_sort_dedup_patch.
// wstatus[t] = SE_DECIDED / SE_DECIDED_XA: desc[t] and reqs[t] (none for the unmapped record, desc.req = -3) are written as
// se_simple_kernel writes them, else only wstatus[t].  d_xa_reqs and d_xa_cnt given (and max_XA_hits <= PW_XA_CAP): a read whose line
// carries XA entries (src/bwamem_extra.c:98-118) is decided too: xa_cnt[t] entries, their requests (pad = the hit's contig) at
// xa_reqs[t * PW_XA_CAP ..], desc[t].flag bits 16-19 = the count.  Without them such a read gets SE_HOST_XA.
// Reads with supplementary lines (src/bwamem.c:1015-1032, without MEM_F_ALL and without ALT hits): with the side arrays of SeLines a read
// whose record has 2 .. SE_LINES_CAP lines is decided with SE_DECIDED_LINES instead of SE_HOST_SUPP.  n_lines[t] lines in list order;
// line j of work item t in slot x = t * SE_LINES_CAP + j: desc[x] (flag: 0 for line 0, supp_flag behind it, the XA count in bits 16-19;
// mapq after the cap of :1029; req: the line's request relative to the read's first, requests laid out as [line 0, its XA entries,
// line 1, its XA entries, ...]), reqs[x], xa_cnt[x] and the XA requests at xa_reqs[x * PW_XA_CAP ..].  desc[t] / reqs[t] / xa_cnt[t] of
// the launch are not written for such a read.  xa_reqs = nullptr (or max_XA_hits > PW_XA_CAP): a read with 1 .. max_XA_hits XA entries
// on any line gets SE_HOST_XA.  More than SE_LINES_CAP lines: SE_HOST_SUPP.  Without the arrays (desc = nullptr) nothing changes.
#define SE_DECIDED_LINES 17
#define SE_LINES_CAP 4
extern "C" int mi355x_se_lines_cap(void);
struct SeLines {
	SamDesc *desc = nullptr;
	AlnReq *reqs = nullptr;
	uint8_t *n_lines = nullptr, *xa_cnt = nullptr;
	AlnReq *xa_reqs = nullptr;
	int supp_flag = 0x800;   // 0x100 under MEM_F_NO_MULTI: the 0x10000 of :1028 as mem_aln2sam prints it; the line is a supplementary one all the same
	int keep_mapq = 0;       // MEM_F_KEEP_SUPP_MAPQ
};
inline void se_lines_options(const mem_opt_t *opt, SeLines &S)
{
	S.supp_flag = opt->flag & MEM_F_NO_MULTI ? 0x100 : 0x800;
	S.keep_mapq = opt->flag & MEM_F_KEEP_SUPP_MAPQ ? 1 : 0;
}
void launch_se_wave(void *stream, const PairParams &P, int n_work, const int *d_work, const DevReg *d_lists, const int *d_loff, const uint8_t *d_ann_alt,
                    const double *d_ltab, uint8_t *d_wstatus, AlnReq *d_reqs, SamDesc *d_desc, AlnReq *d_xa_reqs = nullptr, uint8_t *d_xa_cnt = nullptr,
                    const SeLines *lines = nullptr);

// ---- the units a wave kernel decided, into a CIGAR-and-SAM job of their own (wave_scatter_kernel, se_wave_kernel.hip) ----
// ends = 2: pair_wave_kernel's work list, 1: se_wave_kernel's.  dst[t] = first request of work item t's unit in `reqs`, or < 0 (not in
// the job); per end [the end's request (an unused slot for the unmapped single-end record), its min(xa_cnt, PW_XA_CAP) XA requests, none
// without d_xa_cnt]; desc[ends * work[t] + e]: chunk-wide, by read; clear_n > 0: reads clear_r0 .. + clear_n of desc are marked "not
// the device's" first
void launch_wave_job_scatter(void *stream, int ends, int n_work, const int *d_work, const int *d_dst, const AlnReq *d_w_reqs, const SamDesc *d_w_desc,
                             const AlnReq *d_xa_reqs, const uint8_t *d_xa_cnt, AlnReq *d_reqs, SamDesc *d_desc, int clear_r0, int clear_n);
// its sibling for se_wave_kernel's reads of several lines (ends = 1) and pair_wave_kernel's pairs reported end by end (ends = 2, the
// side arrays by (item, end): end 0's lines, then end 1's): the requests of work item t with dst[t] >= 0 go to
// reqs[dst[t] ..] as [line 0, its XA entries, line 1, ...] from the side arrays (device.h: SeLines); the line descriptors stay where
// the kernel wrote them (sam_lines_kernel reads them there), and the chunk-wide descriptor of the read stays "not the device's"
void launch_lines_job_scatter(void *stream, int ends, int n_work, const int *d_dst, const uint8_t *d_n_lines, const AlnReq *d_lreq, const uint8_t *d_lxcnt,
                              const AlnReq *d_lxreq, AlnReq *d_reqs);

// ---- the redundancy pass of mem_sort_dedup_patch on the raw region lists (dedup_kernel.hip) ----
#define DD_MAXREG 512             // regions per read dedup_wave_kernel takes (its LDS footprint)
extern "C" int mi355x_dedup_maxreg(void);
// status codes of the stage (the numbers of the SE_* codes where the test is the same)
#define DD_HOST 0                 // not looked at
#define DD_TAKEN 1                // keep[reg_pos[i] .. + m[i]) lists the survivors in the reference's final order
#define DD_HOST_MAXREG 3          // more than DD_MAXREG regions
#define DD_HOST_PATCH 4           // two regions mem_patch_reg would align across
struct DedupParams {
	int64_t l_pac;
	int max_chain_gap, w;
	float mask_level_redun;
	int pad;
};
DedupParams dedup_params(const mem_opt_t *opt, int64_t l_pac);
inline size_t dedup_list_ints(int n_reads) { return (size_t)n_reads + 4; }   // the wave kernel's reads, and their number behind them
// d_packed / d_reg_pos / d_nregs as launch_reg_pack leaves them (read only).  Per read: status[i], m[i] (-1: declined); per region slot:
// keep[reg_pos[i] + k], k < m[i] = the place in the read's raw list of the k-th region of mem_sort_dedup_patch's result.  Nothing else of
// keep is written.  d_list: dedup_list_ints(n_reads) ints of scratch.  Two launches: a lane per read up to PR_MAXREG regions (which also
// lists the longer reads), then a wavefront per listed read.
void launch_dedup(void *stream, const DedupParams &D, int n_reads, const DevReg *d_packed, const int *d_reg_pos, const int *d_nregs, uint8_t *d_status,
                  int *d_m, int *d_keep, int *d_list);

// ---- mate-rescue local alignment on the device (msw_kernel.hip) ----
struct MswReq {                  // one ksw_align2() call of mem_matesw (src/bwamem_pair.c:150-177)
	int64_t rb, re;              // target window in the doubled coordinate, already clipped to the contig
	int32_t read;                // the mate to align (index into the batch)
	int32_t is_rev;              // align its reverse complement
};
struct MswRes { int32_t score, te, qe, score2, te2, tb, qb, flags; };   // kswr_t + flags (1 = recompute on the host)
struct MswParams {
	int64_t l_pac;
	uint32_t slo[4];             // scores of target base t against query codes 0..3, one byte each
	int s4[4];                   // ... against query code 4 (N)
	int o_del, e_del, o_ins, e_ins;
	int a, min_seed_len;
	int max_sc, shift;           // max(mat) and -min(mat) as the striped kernel derives them (src/ksw.c:83-88)
};
size_t msw_lds_bytes(int max_len);
// d_rows: scratch of n_req * (longest window) u16
// h_req / h_len (read lengths) / h_list / d_list (2 n_req ints each) / d_tail (msw_tail_ints(n_req) ints) given: requests next to each
// other for the same mate and orientation are aligned two per quad in packed 16-bit arithmetic (msw2_kernel), and the alignments that
// need the reverse pass get it in a launch of their own behind it, sorted by class and again two per quad (msw_rev2_kernel;
// MPIBWA_MSW_REV2=0: one per quad, msw_tail_kernel); otherwise every request on its own
void launch_msw(void *stream, const MswParams &P, int n_req, const MswReq *d_req, const uint8_t *d_seq, const int64_t *d_off, const int *d_len,
                const uint8_t *d_pac, MswRes *d_res, uint16_t *d_rows, int max_len, const MswReq *h_req = nullptr, const int *h_len = nullptr,
                int *h_list = nullptr, int *d_list = nullptr, int *d_tail = nullptr);
// d_tail: the lists of the second pass, all of it sized before the launch — the class offsets in members and in work items
// (MSW_OFF_INTS each), the request indices sorted by class, the class bytes, the sort's histograms per block of MSW_SORT_CHUNK requests
#define MSW_NCLS 48               // 16 segment lengths of the reverse pass x 3 score classes
#define MSW_SORT_CHUNK 4096
#define MSW_OFF_INTS 64
inline size_t msw_tail_ints(size_t n_req)
{
	return 2 * MSW_OFF_INTS + n_req + (n_req + 3) / 4 + (n_req + MSW_SORT_CHUNK - 1) / MSW_SORT_CHUNK * MSW_NCLS;
}
// what the second pass of the last launch_msw with this d_tail ran (waits for nothing: call it behind the stream): pairs of
// msw_rev2_kernel, alone-riders, work items of a register launch, of the general launch
void msw_tail_counts(const int *d_tail, uint64_t out[4]);
MswParams msw_params(const mem_opt_t *opt, int64_t l_pac);
// Can mate rescue run on the device under these options?  Not with o_ins = 0: the reference's lazy-F loop then ends after the first
// position of every segment (its exit test f - e_ins <= max(h, f) - (o_ins + e_ins) holds at once), a carry across a segment border
// raises that one position only, and the kernels' Ffull would carry it on.  Every other gap penalty is the kernels'.
bool msw_on_device(const mem_opt_t *opt);

// ---- seed enumeration between SMEM and SA lookup (fm_kernels.hip) ----
// per read: sort intervals by info, l_rep (src/bwamem.c:265-272) and the number of SA rows to look up
void launch_seed_prep(void *stream, int n_reads, int cap, uint64_t *d_intv, const int *d_nintv, int max_occ, int *d_nseeds, int *d_lrep);
// per read: write the SA rows and (qbeg,len) of every seed in mem_chain's order (src/bwamem.c:273-283)
void launch_seed_enum(void *stream, int n_reads, int cap, const uint64_t *d_intv, const int *d_nintv, int max_occ,
                      const int64_t *d_seed_off, uint64_t *d_rows, int32_t *d_qbeg_len);

// ---- BGZF blocks on the device (bgzf_kernel.hip, bgzf_stage.hip) ----
#define BGZF_DEV_INPUT 0xff00     // text per block (sampost.cpp: BGZF_INPUT)
// block b = d_text[d_cut[b] .. d_cut[b + 1]) (1 .. BGZF_DEV_INPUT bytes; d_text has 16 bytes of slack behind the last block) into the 64-KiB
// slot d_slots + b * 65536 as one complete BGZF block of d_sizes[b] bytes; d_meta[1] += the blocks written stored.  `grid` workgroups of
// one wavefront, each with BGZF_DEV_INPUT 16-bit words of d_tokens.  With d_n_blocks the number of blocks is read on the device (at most
// n_blocks, which then only sizes the launch): the BAM stage makes its cuts there.
void launch_bgzf_deflate(void *stream, const uint8_t *d_text, const uint32_t *d_cut, int n_blocks, uint8_t *d_slots, uint32_t *d_sizes,
                         uint16_t *d_tokens, int grid, unsigned long long *d_meta, const uint32_t *d_n_blocks = nullptr);
// the slots closed up into d_out; d_meta[0] = the bytes
void launch_bgzf_gather(void *stream, const uint8_t *d_slots, const uint32_t *d_sizes, int n_blocks, uint8_t *d_out, unsigned long long *d_meta,
                        const uint32_t *d_n_blocks = nullptr);
void release_bgzf_contexts();     // the idle ones' buffers and streams (mi355x_finalize)
// ---- SAM text to BAM records on the device (bam_kernel.hip, bam_stage.hip; bam_util.h) ----
#define BAM_DEV_TEXT (24u << 20)                 // SAM text per piece
#define BAM_DEV_LINES (BAM_DEV_TEXT / 64)        // lines per piece: a piece of shorter lines goes to the host
#define BAM_DEV_BLOCKS 512                       // BGZF blocks per piece (bgzf_stage.hip: BZ_PIECE)
#define BAM_DEV_BYTES (BAM_DEV_BLOCKS * BGZF_DEV_INPUT)   // BAM bytes per piece
#define BAM_DEV_CHUNK 4096                       // text per workgroup of the line-start kernels
struct BamDevCtl {          // one per piece, in device memory; zeroed but for err before the launch
	uint32_t n_lines;       // of the piece
	uint32_t n_write;       // n_lines, or 0 when the piece is the host's (an error, a declined line, too many lines, bytes or blocks)
	uint32_t err;           // the smallest offset of a malformed line, 0xffffffff: none
	uint32_t decline;
	uint32_t bam_bytes;     // of the records
	uint32_t n_blocks;      // of the cuts
};
struct BamDevBufs {
	const uint8_t *text; uint32_t text_len;      // whole lines, the last byte is '\n'
	const void *contigs;                         // bam_util.h's blob
	uint32_t *chunk_cnt;                         // text_len / BAM_DEV_CHUNK + 2
	uint32_t *line_start;                        // BAM_DEV_LINES + 1
	void *plan;                                  // BAM_DEV_LINES x bam::LinePlan
	uint32_t *group;                             // BAM_DEV_LINES / 64 + 1
	uint32_t *rec_off;                           // BAM_DEV_LINES + 1
	uint32_t *next;                              // BAM_DEV_LINES
	uint8_t *bam;                                // BAM_DEV_BYTES + 16
	uint32_t *cut;                               // BAM_DEV_BLOCKS + 1
	BamDevCtl *ctl;
};
// the records of the piece into B.bam, their offsets into B.rec_off (all of it queued on the stream, nothing comes back)
void launch_bam_encode(void *stream, const BamDevBufs &B);
// the blocks' cuts of the records into B.cut and B.ctl->n_blocks
void launch_bam_cuts(void *stream, const BamDevBufs &B);
size_t bam_plan_bytes();
void release_bam_contexts();      // the idle ones' buffers and streams (mi355x_finalize)
// ---- BGZF blocks inflated on the device (bgzf_inflate_kernel.hip, bgzf_in_stage.hip) ----
// block b = d_comp[d_blk_off[b] .. d_blk_off[b + 1]) (a whole BGZF block: header, deflate stream, CRC32, ISIZE; d_comp holds comp_len bytes)
// to d_text[d_text_off[b] .. d_text_off[b + 1]) (the ISIZEs' prefix sums, below text_cap); d_status[b] = 0 or inflate_util.h's error.
// n_blocks workgroups of one wavefront.
void launch_bgzf_inflate(void *stream, const uint8_t *d_comp, uint32_t comp_len, const uint32_t *d_blk_off, const uint32_t *d_text_off, int n_blocks,
                         uint8_t *d_text, uint32_t text_cap, uint32_t *d_status);
void release_bgzf_in_contexts();  // the idle ones' buffers and streams (mi355x_finalize)
// ---- a BAM file to coordinate order on the device (bam_sort_kernel.hip, bam_sort_stage.hip; bam_sort_util.h) ----
// d_u: the whole inflated stream (bsort::BAM_SORT_SLACK bytes behind its end), block b = d_u[d_text_off[b] .. d_text_off[b + 1]), records
// from h_end on.  count: d_cnt[0 .. n_blk] = the records of every block's own chain (d_cnt[n_blk] = 0), *d_bad = 1 when a chain meets a
// malformed record or does not end at its block's end (the caller zeroes it).  scan: d_first[0 .. n_blk] = their exclusive sums.
// write: record i's offset in d_u, size and packed key.  All of it queued on the stream.
void launch_bam_sort_count(void *stream, const uint8_t *d_u, const uint64_t *d_text_off, int n_blk, uint64_t h_end, int32_t n_ref, uint32_t *d_cnt, uint32_t *d_bad);
void launch_bam_sort_scan(void *stream, void *d_tmp, size_t tmp_bytes, const uint32_t *d_cnt, uint32_t *d_first, int n_blk);
void launch_bam_sort_write(void *stream, const uint8_t *d_u, const uint64_t *d_text_off, int n_blk, uint64_t h_end, int32_t n_ref, const uint32_t *d_first,
                           uint64_t *d_off, uint32_t *d_size, uint64_t *d_key);
size_t bam_sort_temp_bytes(uint32_t n_rec, int n_blk);   // hipCUB's room for the scans and the sort
// the order: d_idx2[i] = the record that sorts to place i (stable, over the key's `bits` lowest bits), d_ssize[i] = its size (d_ssize[n_rec] = 0),
// d_dst[0 .. n_rec] = the exclusive sums of those: where it stands in the sorted stream.  d_dst may be d_key: the keys are done with by then.
void launch_bam_sort_order(void *stream, void *d_tmp, size_t tmp_bytes, uint32_t n_rec, int bits, const uint64_t *d_key, uint64_t *d_key2, uint32_t *d_idx,
                           uint32_t *d_idx2, const uint32_t *d_size, uint32_t *d_ssize, uint64_t *d_dst);
// sorted records r0 .. r1 - 1, as far as they lie in [lo, hi) of the sorted stream, back to back into d_piece[0 .. hi - lo)
void launch_bam_sort_gather(void *stream, const uint8_t *d_u, const uint64_t *d_off, const uint32_t *d_idx, const uint64_t *d_dst, uint32_t n_rec, uint32_t r0,
                            uint32_t r1, uint64_t lo, uint64_t hi, uint8_t *d_piece);
void release_bam_sort_contexts(); // the sort buffers and streams, unless a sort is running (mi355x_finalize)
// ---- the BAI index of a coordinate-sorted stream on the device (bam_index_kernel.hip, bam_sort_stage.hip; bam_index_util.h) ----
// Record i of the file (i < n_rec) stands at u[off[order ? order[i] : i]] and at place_base + place[i] of the indexed file's stream,
// whose blocks start at cut[0 .. n_cut] (cut[n_cut]: the stream's end).  keys (or none): the packed sort keys in file order, checked.
// *bad: the smallest off of a record that fails the call (the caller sets it to ~0).  Virtual offsets are block << 16 | offset in block.
struct BamIndexBufs {
	const uint8_t *u; const uint64_t *off; const uint32_t *order; const uint64_t *place; uint64_t place_base; const uint64_t *cut; uint64_t n_cut;
	uint32_t n_rec; int32_t n_ref; const uint64_t *keys; uint64_t end_v;   // end_v: v1 of the last record
	// per record: the run key, v0, ref << 32 | end and its inclusive maxima, beg, mapped (n_rec + 1) and its exclusive sums (n_rec + 1),
	// the head flags, the runs' first records and their number
	uint64_t *rb, *v0, *mx, *mxs; uint32_t *beg, *map, *maps; uint8_t *head; uint32_t *rs, *n_sel;
	// per contig (n_ref + 1): four words of statistics, n_intv and its exclusive sums
	uint64_t *stat; uint32_t *n_intv, *woff;
	// per run: key and number, both sorted; the chunks in sorted order.  per window: v0 of its first record or BAI_NO_RECORD
	uint64_t *rk, *rk2; uint32_t *ri, *ri2; uint64_t *rbeg, *rend, *io;
	unsigned long long *bad; void *tmp; size_t tmp_bytes;
};
size_t bam_index_temp_bytes(uint32_t n_rec, int32_t n_ref, uint32_t n_runs);   // hipCUB's room
// the record pass, the scans, the runs' heads (rs, *n_sel), the contigs' statistics, n_intv and woff (woff[n_ref]: all windows)
void launch_bam_index_records(void *stream, const BamIndexBufs &B);
// once the host knows the runs and the windows: rk2, rbeg, rend (sorted by contig and bin, stably) and io
void launch_bam_index_runs(void *stream, const BamIndexBufs &B, uint32_t n_runs, uint32_t n_win);
// the calling thread on the device of the resident index, or, before any index, on device 0 after the checks of mi355x_init
void use_device();

SmemParams smem_params(const mem_opt_t *opt);
int clamp_band(const mem_opt_t *opt, int qlen, int w, int end_bonus);

} // namespace mbw
#endif
