/* mpibwa_amd.h — C ABI of the MI355X-native BWA-MEM hot path.
 *
 * This header is the drop-in boundary for mpiBWA's alignment call
 *     mem_process_seqs(opt, bwt, bns, pac, n_processed, n, seqs, pes0)
 * (reference: src/bwamem.h:134, called from src/mainParallel.c:1314, :2355,
 * :3093 and src/mainParallelByChromosome.c:1249, :2502, :3407).
 *
 * Everything here is plain C: pointers, sizes, PODs.  No torch / HIP types
 * cross the boundary.  The struct layouts below are re-declared from the
 * reference's documented x86-64 layouts so that a host program compiled
 * against the reference headers can pass its own objects unchanged:
 *     mem_opt_t     src/bwamem.h:25-57   (168 bytes)
 *     mem_pestat_t  src/bwamem.h:81-85   (32 bytes)
 *     bseq1_t       src/bwa.h:30-33      (48 bytes)
 *     bwt_t         src/bwt.h:46-58      (1120 bytes incl. cnt_table)
 *     bntann1_t     src/bntseq.h:41-48   (40 bytes)
 *     bntamb1_t     src/bntseq.h:50-54   (16 bytes)
 *     bntseq_t      src/bntseq.h:56-64   (48 bytes)
 * Sizes and field offsets are checked at build time by static asserts in
 * mpibwa_amd/csrc/abi_check.cpp (C++) and tests/abi_check.c (plain C).
 */
#ifndef MPIBWA_AMD_H
#define MPIBWA_AMD_H

#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- flag bits of mem_opt_t::flag (src/bwamem.h:14-23) ---- */
#define MEM_F_PE             0x2
#define MEM_F_NOPAIRING      0x4
#define MEM_F_ALL            0x8
#define MEM_F_NO_MULTI       0x10
#define MEM_F_NO_RESCUE      0x20
#define MEM_F_REF_HDR        0x100
#define MEM_F_SOFTCLIP       0x200
#define MEM_F_SMARTPE        0x400
#define MEM_F_PRIMARY5       0x800
#define MEM_F_KEEP_SUPP_MAPQ 0x1000

typedef uint64_t bwtint_t;

typedef struct {
	int a, b;
	int o_del, e_del;
	int o_ins, e_ins;
	int pen_unpaired;
	int pen_clip5, pen_clip3;
	int w;
	int zdrop;
	uint64_t max_mem_intv;
	int T;
	int flag;
	int min_seed_len;
	int min_chain_weight;
	int max_chain_extend;
	float split_factor;
	int split_width;
	int max_occ;
	int max_chain_gap;
	int n_threads;
	int chunk_size;
	float mask_level;
	float drop_ratio;
	float XA_drop_ratio;
	float mask_level_redun;
	float mapQ_coef_len;
	int mapQ_coef_fac;
	int max_ins;
	int max_matesw;
	int max_XA_hits, max_XA_hits_alt;
	int8_t mat[25];
} mem_opt_t;

typedef struct {
	int low, high;
	int failed;
	double avg, std;
} mem_pestat_t;

typedef struct {
	int l_seq, id;
	char *name, *comment, *seq, *qual, *sam;
} bseq1_t;

typedef struct {
	bwtint_t primary;
	bwtint_t L2[5];
	bwtint_t seq_len;
	bwtint_t bwt_size;      /* in 32-bit words */
	uint32_t *bwt;          /* occ-interleaved BWT, 64 B per 128 bases */
	uint32_t cnt_table[256];
	int sa_intv;
	bwtint_t n_sa;
	bwtint_t *sa;
} bwt_t;

typedef struct {
	int64_t offset;
	int32_t len;
	int32_t n_ambs;
	uint32_t gi;
	int32_t is_alt;
	char *name, *anno;
} bntann1_t;

typedef struct {
	int64_t offset;
	int32_t len;
	char amb;
} bntamb1_t;

typedef struct {
	int64_t l_pac;
	int32_t n_seqs;
	uint32_t seed;
	bntann1_t *anns;
	int32_t n_holes;
	bntamb1_t *ambs;
	FILE *fp_pac;
} bntseq_t;

/* in-memory index handle, same fields as the reference's bwaidx_t
 * (src/bwa.h:20-28) so `.map` images can be attached in place. */
typedef struct {
	bwt_t    *bwt;
	bntseq_t *bns;
	uint8_t  *pac;
	int       is_shm;
	int64_t   l_mem;
	uint8_t  *mem;
} bwaidx_t;

/* ------------------------------------------------------------------ */
/* The drop-in entry point (replaces src/bwamem.c:1205-1234).          */
/*                                                                     */
/* Same argument meaning, same in/out contract on seqs[] (seq[] is     */
/* overwritten with nt4 codes, seqs[i].sam is malloc()ed and owned by  */
/* the caller), same stderr messages, failures abort.  The index       */
/* (bwt,bns,pac) must have been uploaded with mi355x_index_upload()    */
/* first; calling without a usable MI355X device aborts loudly — there */
/* is no CPU fallback.                                                 */
/*                                                                     */
/* Threads: the function may be called from several threads at once    */
/* (same index, disjoint seqs[]).  Up to eight calls run side by side  */
/* — the first half of a call is bound by the GPU, the second by the   */
/* host, so chunk i+1 overlaps chunk i — and further callers wait for  */
/* a free slot (calls in flight on overlapping seqs[] abort).          */
/* The reference's own function is re-entrant in the same way (it     */
/* only reads opt and the index).                                      */
/* ------------------------------------------------------------------ */
void mem_process_seqs(const mem_opt_t *opt, const bwt_t *bwt, const bntseq_t *bns, const uint8_t *pac,
                      int64_t n_processed, int n, bseq1_t *seqs, const mem_pestat_t *pes0);

/* option / scoring helpers used by the caller's CLI parsing
 * (src/bwamem.c:48-84, src/bwa.c:109-119, src/bwa.c:16-17). */
mem_opt_t *mem_opt_init(void);
void bwa_fill_scmat(int a, int b, int8_t mat[25]);
extern int  bwa_verbose;
extern char bwa_rg_id[256];
/* read-group / extra header lines of the caller's CLI (src/bwa.c:431-476; used by src/mainParallel.c:356, :368, :373):
 * bwa_set_rg() returns the unescaped "@RG..." line (malloc()ed) and fills bwa_rg_id with its ID, or 0 if malformed;
 * bwa_insert_header() appends an unescaped '@' line to the header text (realloc()ed) and returns it. */
char *bwa_set_rg(const char *s);
char *bwa_insert_header(const char *s, char *hdr);

/* index attach / load (src/bwa.c:262-345: bwa_idx_load_from_disk, bwa_mem2idx) */
bwaidx_t *bwa_idx_load_from_disk(const char *prefix, int which);
int       bwa_mem2idx(int64_t l_mem, uint8_t *mem, bwaidx_t *idx);
void      bwa_idx_destroy(bwaidx_t *idx);
/* `.map` packer (src/bwa.c:347-386, used by mpiBWAIdx src/pidx.c:52-63): turns a disk-loaded index into one contiguous
 * malloc()ed image [bwt_t][bwt words][sa][bntseq_t][ambs][anns][name\0anno\0...][pac] and re-attaches idx to it. */
int       bwa_idx2mem(bwaidx_t *idx);
/* mpiBWAIdx in one call: load <prefix>.{bwt,sa,ann,amb,pac}, pack, write the image to map_path (pointer fields zeroed). */
int       mi355x_write_map(const char *prefix, const char *map_path);

/* ---- MI355X-specific additions (no reference equivalent) ---- */

/* Select device `local_rank`, re-home the FM-index (64-B aligned occ blocks),
 * the sampled SA and the 2-bit pac into HBM.  Returns 0 on success; aborts if
 * no gfx950 device is usable. */
int  mi355x_index_upload(int local_rank, const bwt_t *bwt, const bntseq_t *bns, const uint8_t *pac);
/* Device pointers + sizes of the three index arrays, for the RCCL broadcast
 * done by the host program (rank 0 uploads, others call mi355x_index_alloc
 * then receive into these buffers). */
int  mi355x_index_alloc(int local_rank, const bwt_t *bwt_meta, const bntseq_t *bns);
int  mi355x_index_buffers(void **d_bwt, size_t *bwt_bytes, void **d_sa, size_t *sa_bytes, void **d_pac, size_t *pac_bytes);
/* broadcast path: copy between a caller-owned device buffer and index buffer `which` (0 occ blocks, 1 SA, 2 pac);
 * once all three are filled, mi355x_index_commit() expands the dense SA and makes the index usable */
int  mi355x_index_d2d(int which, void *ext_device_ptr, size_t bytes, int to_index);
int  mi355x_index_commit(void);
void mi355x_finalize(void);

/* One call per rank after the index has been attached (replaces the per-rank copy of src/parallel_aux.c:1779-1830):
 * selects GPU `local_rank`; with comm == NULL or comm->size == 1 the index is uploaded from idx; otherwise rank 0 of
 * the communicator uploads its copy and the occ blocks, the sampled SA and pac reach the other ranks' GPUs by
 * ncclBroadcast (RCCL over xGMI, in pieces), after which every rank expands its dense SA and jump table.
 * The library does not link MPI: the caller lends its own transport for the 128-byte RCCL bootstrap id. */
typedef struct {
	int rank, size;                                                  /* among the ranks that share the broadcast (one per GPU) */
	void (*bcast)(void *buf, size_t bytes, int root, void *user);    /* host-memory broadcast, e.g. a wrapper of MPI_Bcast */
	void *user;
} mi355x_comm_t;
int  mi355x_init(int local_rank, const bwaidx_t *idx, const mi355x_comm_t *comm);
/* GPUs visible to this process (a host program that starts more ranks than that lets ranks share a device) */
int  mi355x_device_count(void);
/* compute units of the current device, as the kernel launchers read them to size their grids; 0 on failure */
int  mi355x_device_cus(void);
/* free / total bytes of HBM on the device the index lives on; 0 on success */
int  mi355x_device_memory(size_t *free_bytes, size_t *total_bytes);
/* (re)allocations of device / page-locked work buffers since the library was loaded: they stall every stream of the device, so
 * the number should stand still once every call context has seen its largest chunk */
unsigned long long mi355x_buffer_growths(void);
/* host threads the library uses for this rank's calls (its share of the node's usable CPUs; *ranks_on_node: the ranks it believes
 * share the node, from the launcher's environment).  mi355x_init prints it and refuses to start with fewer than 2. */
int  mi355x_rank_host_threads(int *ranks_on_node);
/* device-computed checksums of the three resident index arrays (occ blocks, sampled SA, pac): mi355x_init compares every rank's
 * with rank 0's after its broadcast and ends the run on a difference; a host that broadcasts by other means does the same with this */
int  mi355x_index_checksums(uint64_t out[3]);
/* mem_process_seqs calls the library runs side by side at most (further callers wait; fewer are admitted while their work buffers
 * would not fit in HBM): the most worker threads a chunk loop has use for */
int  mi355x_max_calls(void);
/* The first-use cost of `n_calls` call contexts (work buffers on the device and page-locked on the host, streams, the host thread
 * pool, the kernels' code objects: 1-2 s per context otherwise paid by the first chunks of the loop the reference brackets with
 * MPI_Wtime, src/mainParallel.c:1238-1319) paid now: n_calls mem_process_seqs calls side by side on n_reads reads of read_len
 * bases sampled from the reference itself, text thrown away.  opt / bwt / bns / pac: what the chunk loop will pass.  A caller
 * with other work left before its loop runs this on a thread of its own meanwhile.  n_calls is also taken as what the caller
 * will keep in flight: with three or more, its calls run in their many-callers mode from the first one on (otherwise the library
 * finds out by itself after two of them).  Returns the seconds it took. */
double mi355x_prewarm(const mem_opt_t *opt, const bwt_t *bwt, const bntseq_t *bns, const uint8_t *pac, int n_reads, int read_len, int n_calls);
/* seconds spent in the RCCL broadcast of the last mi355x_init (0 when none took place) */
double mi355x_init_bcast_seconds(void);

/* own bwa-compatible index builder (formats of src/bwt.c:385-462,
 * src/bntseq.c:66-96,275-328). Writes prefix.{pac,ann,amb,bwt,sa}. */
int  mi355x_index_build(const char *fasta, const char *prefix);
/* same .bwt/.sa, built in HBM (radix sort + prefix doubling on the device) from an N-free forward pac
 * of l_pac bases; used for GRCh38-sized synthetic references.  *seconds = device build time. */
int  mi355x_index_build_gpu(int device, const uint8_t *pac, int64_t l_pac, const char *prefix, double *seconds);

/* ---- stage-level entry points (used by tests/bench for kernel parity and
 *      roofline measurement; each runs ONLY the named HIP kernel) ---- */

/* SMEM seeding (mem_collect_intv, src/bwamem.c:114-162) for n reads.
 * seqs: concatenated nt4 bytes, off[n+1] offsets.  Output: per read up to
 * `cap` intervals (x0,x1,x2,info) = 4 x uint64 each, count in n_out[i],
 * sorted by info.  Returns 0, or -1 if some read overflowed `cap`. */
int mi355x_smem_batch(const mem_opt_t *opt, int n, const uint8_t *seqs, const int64_t *off,
                      int cap, uint64_t *intv_out, int *n_out, double *kernel_ms, uint64_t *algo_bytes);
/* Suffix-array lookup (bwt_sa, src/bwt.c:86-96) for n BWT rows. */
int mi355x_sa_batch(int n, const uint64_t *k, uint64_t *sa_out, double *kernel_ms, uint64_t *algo_bytes);
/* Same lookups answered from the dense SA that mi355x_index_upload() expands in HBM when memory allows
 * (dense != 0; returns -1 if the table is absent), or by the LF walk (dense == 0). */
int mi355x_sa_batch2(int n, const uint64_t *k, uint64_t *sa_out, double *kernel_ms, int dense);
/* expansion time in ms (0 if not expanded) and, through *bytes, the size of the dense table */
double mi355x_sa_dense_info(size_t *bytes);
/* Banded extension (ksw_extend2, src/ksw.c:380-479) for n independent jobs.
 * q/t: concatenated nt4 bytes; per job 5 ints in out: score,qle,tle,gtle,gscore,max_off (6). */
int mi355x_extend_batch(const mem_opt_t *opt, int n, const uint8_t *q, const int64_t *qoff,
                        const uint8_t *t, const int64_t *toff, const int *w, const int *h0,
                        const int *end_bonus, int *out6, double *kernel_ms, uint64_t *cells);
/* The same through the row loop the chain-to-region kernel runs.  Per job: early[i] != 0 stops the rows as soon as nothing
 * mem_chain2aln reads can change, given the clipping penalty clip[i] — then score, qle, tle, max_off and the local / global
 * decision (gscore <= 0 || gscore <= score - clip) are the reference's, gscore and gtle too when the decision is "global";
 * early[i] == 0: all six outputs are the reference's.  cells[i]: DP cells computed for job i. */
int mi355x_extend_batch2(const mem_opt_t *opt, int n, const uint8_t *q, const int64_t *qoff,
                         const uint8_t *t, const int64_t *toff, const int *w, const int *h0,
                         const int *end_bonus, const int *early, const int *clip, int *out6,
                         uint64_t *cells, double *kernel_ms);

/* Chaining stage (mem_chain + mem_chain_flt, src/bwamem.c:251-385) for n_reads reads given by their seeds
 * (read r owns seeds seed_off[r] .. seed_off[r+1]: rbeg[], and qbeg/len interleaved in qbeg_len[]), computed by
 * chain_kernel (which = 0) or by the library's host path (which = 1).  Output per read from out[out_off[r]]:
 * n_chains (-1 = the kernel leaves the read to the host), then per kept chain rid, n_seeds, far_beg, far_end,
 * rmax0, rmax1, frac_rep (float bits) and n_seeds x (rbeg, qbeg, len) in the order mem_chain2aln visits them.
 * Returns the number of int64 written, or -1 if out_cap is too small. */
int64_t mi355x_chain_batch(const mem_opt_t *opt, const bntseq_t *bns, int n_reads, const int *lens, const int *l_rep,
                           const int64_t *seed_off, const uint64_t *rbeg, const int32_t *qbeg_len, int which,
                           int64_t *out, int64_t out_cap, int64_t *out_off);

/* Chain -> alignment regions (mem_chain2aln, src/bwamem.c:632-786, applied to the chains of a read in order as mem_align1_core does)
 * for n_reads reads given as nt4 codes (reads[off[r] .. off[r+1])) and their chains as mem_chain_t holds them after mem_chain_flt and
 * mem_flt_chained_seeds: read r has n_chains[r] chains, chain c has rid chain_rid[c], frac_rep chain_frac[c] and chain_nseeds[c] seeds,
 * all of them back to back, seed s = (seed_rbeg[s], seed_qbeg[s], seed_len[s], seed_score[s]) in the chain's array order.  The
 * library's own packing, c2a_kernel and its chain groups and the region packing run as the pipeline runs them, on the resident index
 * (mi355x_index_upload).  heavy_t: reads with more chains than that are split into independent groups of chains (0: never);
 * early: 1 = no-DP closed form and early row stops (the product's default), 0 = every row of the reference, 2 = both, differences
 * counted; layout 0 = the slots of device-chained reads (read r owns a sparse run of slots), 1 = those of host-chained reads (dense,
 * behind the others).  Output per read from out[out_off[r]]: n_regs, then per region rb, re, qb, qe, rid, score, truesc, w, seedcov,
 * seedlen0, frac_rep (float bits).  stat4: DP cells, extensions, extensions without DP, extensions that differ (early = 2);
 * *n_units: units of the groups path.  Returns the number of int64 written, or -1 if out_cap is too small. */
int64_t mi355x_c2a_batch(const mem_opt_t *opt, const bntseq_t *bns, int n_reads, const uint8_t *reads, const int64_t *off,
                         const int *n_chains, const int *chain_rid, const float *chain_frac, const int *chain_nseeds,
                         const int64_t *seed_rbeg, const int *seed_qbeg, const int *seed_len, const int *seed_score,
                         int heavy_t, int early, int layout, int64_t *out, int64_t out_cap, int64_t *out_off,
                         uint64_t *stat4, int *n_units);

/* Final global re-alignment (mem_reg2aln's loop src/bwamem.c:1106-1122 around bwa_gen_cigar2 src/bwa.c:121-207 and
 * ksw_global2 src/ksw.c:504-606) for n_req regions [rb,re) x [qb,qe) of read `read` (nt4 codes, read r =
 * reads[off[r]..off[r+1])) against the 2-bit packed reference `pac` of l_pac bases, computed by aln_kernel.
 * which: 0 = the product's dispatch (no-DP shortcut / narrow-band instantiation with hand-off to the full-size one),
 * 1 = DP requests straight to the full-size instantiation.
 * Per request out_hdr gets score, NM, n_cigar, md_len, flags (1 = the device declined: band matrix beyond its budget);
 * cigar (BAM-encoded u32) goes to cigar_out[cigar_cap * i ..], MD text to md_out[md_cap * i ..].
 * read[i] == -1 marks an unused slot of the request array; it, and a request that no instantiation of the kernel answered,
 * comes back with flags = -1 (the headers are filled with -1 before the launch).
 * mi355x_global_batch_counts: of the last call, the final lengths of the three request lists (no-DP, narrow band, full size)
 * and the bytes of the result pool handed out. */
int mi355x_global_batch(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, int n_reads, const uint8_t *reads,
                        const int64_t *off, int n_req, const int64_t *rb, const int64_t *re, const int *read,
                        const int *qb, const int *qe, const int *w, const int *truesc, int which,
                        int *out_hdr5, uint32_t *cigar_out, int cigar_cap, char *md_out, int md_cap, double *kernel_ms);
void mi355x_global_batch_counts(uint64_t out[4]);

/* Pairing decisions of mem_sam_pe (src/bwamem_pair.c:250-393 with mem_sort_dedup_patch src/bwamem.c:437-489, the test of
 * mem_matesw :118-128, mem_mark_primary_se src/bwamem.c:493-569, mem_pair :182-243, mem_approx_mapq_se src/bwamem.c:952-976,
 * the XA test of src/bwamem_extra.c:91-110) for n_pairs pairs given by the regions of their ends as phase 1 leaves them
 * (regs: mi355x_pair_maxreg() records of 64 bytes per read — rb, re (int64), qb, qe, rid, score, truesc, w, seedcov, seedlen0 (int32), frac_rep
 * (float), pad; n_regs per read), computed by pair_simple_kernel.  status[k] = 1: the pair is decided — desc (56 bytes per read:
 * rb, re, qb, qe, req, rid, flag, mapq, score, sub) and req (40 bytes per read: rb, re, read, qb, qe, w2, truesc, pad) describe the
 * two records of its paired branch; any other value: the kernel leaves the pair to the library's host path (the value names
 * the test that said so).  Returns 0, or -1 when the kernel cannot use these insert-size statistics. */
int mi355x_pair_maxreg(void);
int mi355x_pair_batch(const mem_opt_t *opt, const bntseq_t *bns, const mem_pestat_t pes[4], int64_t n_processed, int n_pairs,
                      const void *regs, const int *n_regs, int max_len, uint8_t *status, void *desc, void *req);

/* mi355x_pair_batch for a test that looks at everything the kernel writes.  pair_ok: n_pairs bytes, 0 = a pair the host did not pass
 * (the kernel gives it code 2 and marks its requests and descriptors as the host's, nothing else).  status has room for
 * mi355x_pair_stage_room(n_pairs) pairs — n_pairs rounded up to 64, and 64 more — desc and req for twice as many records; every byte of
 * the three is `fill` before the launch and all of it comes back, so what lies behind pair n_pairs - 1 must still hold the pattern.
 * Returns 0, or -1 as mi355x_pair_batch. */
int mi355x_pair_stage_room(int n_pairs);
int mi355x_pair_stage_batch(const mem_opt_t *opt, const bntseq_t *bns, const mem_pestat_t pes[4], int64_t n_processed, int n_pairs,
                            const void *regs, const int *n_regs, const uint8_t *pair_ok, int max_len, int fill, uint8_t *status,
                            void *desc, void *req);

/* The same decisions for the pairs pair_simple_kernel leaves because they need mate rescue, carry more than mi355x_pair_maxreg() regions
 * on an end, or have one end without a region: pair_wave_kernel, a pair per wavefront, up to mi355x_pair_wave_maxreg() regions per end.
 * The entry runs the pipeline's sequence: the host lists the rescue windows (src/bwamem_pair.c:131-150), the mate-rescue kernel aligns
 * them, pair_wave_kernel replays mem_sam_pe with the results (rescue loop :265-276 with mem_matesw :111-180, primary marking, mem_pair,
 * MAPQ with csub, the XA test).  2 n_pairs reads as nt4 codes (read r = reads[off[r] .. off[r+1])); regs: both ends' regions AFTER
 * mem_sort_dedup_patch, 64-byte records back to back (the layout of mi355x_pair_batch), read r owns regs[reg_off[r] .. reg_off[r+1]).
 * status, desc, req: as mi355x_pair_batch returns them; codes besides its own: 0 not handed to the kernel (a list that is not a fixed
 * point of the redundancy pass, more than mi355x_pair_wave_maxreg() regions, an ALT hit, no region on either end), 12 a rescue
 * alignment the replay needs is not on the device, 13 a list grows past mi355x_pair_wave_maxreg(), 14 the outcome depends on the
 * order the reference's unstable sorts give equal keys.  *n_align: local alignments run.  Returns 0, or -1 as mi355x_pair_batch. */
int mi355x_pair_wave_maxreg(void);
int mi355x_pair_wave_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], int64_t n_processed,
                           int n_pairs, const uint8_t *reads, const int64_t *off, const void *regs, const int *reg_off, uint8_t *status,
                           void *desc, void *req, int *n_align);

/* The same sequence with the XA listing on: a pair whose chosen hits carry XA entries (mem_gen_alt, src/bwamem_extra.c:98-118: the
 * hits i, in list order, with secondary_all = the chosen hit and score >= its score * XA_drop_ratio; 1 .. max_XA_hits of them) is
 * decided too, with status 16 instead of code 11.  xa_cnt[2k + e] (2 n_pairs bytes): the entries of end e's record; xa_req
 * (2 n_pairs * mi355x_pair_wave_xa_cap() requests of 40 bytes): entry j of end e at [(2k + e) * cap + j], the request mem_reg2aln would
 * make for that hit, its contig in `pad`.  desc[2k + e].flag carries the count in bits 16-19 and desc[2k + 1].req = 1 + xa_cnt[2k]:
 * the pair's requests in a job are [read 0's, its XA entries', read 1's, its XA entries'], which is how mi355x_sam_batch reads a
 * descriptor with a count (the XA text behind the read group, "name,+-pos,CIGAR,NM;" per entry).  Status 1 still says "decided, both
 * records without XA".  With max_XA_hits beyond the cap the entry behaves as mi355x_pair_wave_batch. */
int mi355x_pair_wave_xa_cap(void);
int mi355x_pair_wave_xa_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], int64_t n_processed,
                              int n_pairs, const uint8_t *reads, const int64_t *off, const void *regs, const int *reg_off, uint8_t *status,
                              void *desc, void *req, int *n_align, void *xa_req, uint8_t *xa_cnt);

/* mi355x_pair_wave_xa_batch with the kernel's side arrays for the pairs mem_sam_pe reports end by end through no_pairing:
 * (src/bwamem_pair.c:371-392: an end without a hit, no pair of hits in a proper orientation and distance, a best pair that scores
 * nothing, an end with a second primary hit of at least T).  status[k] = 17: decided that way instead of code 8 / 9 / 10; a pair
 * without any region is looked at too (status 2 -> 17 with no line).  n_lines[2k + e] = 0 .. mi355x_se_lines_cap(): the lines of end
 * e, the primary hits of at least T in list order (src/bwamem.c:1015-1032 without MEM_F_ALL); 0: the end's record is the unaligned one
 * and has neither descriptor nor request.  Line j of end e sits in slot x = (2k + e) * mi355x_se_lines_cap() + j of line_desc, line_req
 * and line_xa_cnt: flag = 0x40 << e | 1, | 2 when both ends have a top hit of at least T on one contig at a proper distance
 * (src/bwamem_pair.c:382-387), | 0x800 behind the end's first line (0x100 under MEM_F_NO_MULTI), the line's XA count in bits 16-19;
 * mapq is mem_approx_mapq_se of the line's own hit (with its csub), lowered to line 0's behind it unless MEM_F_KEEP_SUPP_MAPQ; sub =
 * max(sub, csub); XA entry i's request at line_xa_req[x * mi355x_pair_wave_xa_cap() + i].  desc.req counts from the pair's first request
 * when they are laid out as [end 0: line 0, its XA entries', line 1, ...; end 1: ...], which is how mi355x_sam_pe_lines_batch reads
 * them; req.read = 2k + e.  desc / req / xa_cnt [2k + e] are not written for such a pair.  More than mi355x_se_lines_cap() lines on an
 * end: 10 as before; line_xa_req == NULL or max_XA_hits beyond the cap: a pair with 1 .. max_XA_hits entries on a line gets 11; a line
 * beyond the per-length or sub_n tables: 6.  xa_req == NULL: the paired branch runs without its XA listing.  Pairs the paired branch
 * decides (1, 16) come back exactly as from mi355x_pair_wave_batch / _xa_batch. */
int mi355x_pair_wave_lines_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], int64_t n_processed,
                                 int n_pairs, const uint8_t *reads, const int64_t *off, const void *regs, const int *reg_off, uint8_t *status,
                                 void *desc, void *req, int *n_align, void *xa_req, uint8_t *xa_cnt, uint8_t *n_lines, void *line_desc,
                                 void *line_req, uint8_t *line_xa_cnt, void *line_xa_req);

/* SAM text of the pairs decided on the device: the CIGAR kernel (aln_kernel) and sam_emit_kernel, queued on one stream as the
 * pipeline queues them, on chosen line descriptors.  2 n_pairs reads as nt4 codes (read r = reads[off[r] .. off[r+1])), their
 * qualities at the same places (or NULL: QUAL is '*'), their names back to back (read r = names[name_off[r] .. name_off[r+1])); the
 * read group is whatever bwa_set_rg() left in bwa_rg_id.  desc: 56 bytes per read (rb, re, qb, qe, req, rid, flag, mapq, score, sub,
 * the layout mi355x_pair_batch returns; req = -3: a record of a pair without any hit, any other req < 0: not a record of the device,
 * and then its mate's is not one either); reqs: the CIGAR requests (40 bytes each: rb, re, read, qb, qe, w2, truesc, pad), pair k owns
 * reqs[req_base[k] .. req_base[k+1]) and desc.req counts from req_base[k].  arena_bytes: 0 = mi355x_sam_arena_bytes(2 n_pairs, longest
 * read), the pipeline's own size; grid_blocks: 0 = the launcher's choice, otherwise a cap on the number of workgroups.
 * out_len[r] >= 0: the record is arena_out[out_off[r] .. + out_len[r]); -1: handed back to the host (CIGAR declined, short fields
 * beyond the staging row, arena full) together with its mate; -2: not a record of the device.  arena_out receives the arena and the
 * 4096 guard bytes behind it, both filled with 0xA5 before the launch; *cursor the bytes the kernel claimed (it may exceed
 * arena_bytes when waves were turned away); hdr_out the result headers of the requests (24 bytes each: score, NM, n_cigar, md_len,
 * pool_off, flags). */
size_t mi355x_sam_arena_bytes(int n_reads, int max_len);
int mi355x_sam_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_pairs, const uint8_t *reads, const int64_t *off,
                     const uint8_t *quals, const char *names, const int *name_off, const void *desc, const void *reqs, const int *req_base,
                     size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off, uint8_t *arena_out,
                     unsigned long long *cursor, void *hdr_out);

/* Decisions of the single-end branch of worker2 (src/bwamem.c:1187-1196: mem_mark_primary_se with id = n_processed + i, the walk of
 * mem_reg2sam :1003-1049, mem_approx_mapq_se :952-976, with mem_sort_dedup_patch :437-489 and the XA test of src/bwamem_extra.c:91-110)
 * for n_reads reads given by their regions as phase 1 leaves them (regs, n_regs, desc, req: the layouts of mi355x_pair_batch, one
 * descriptor and one request per read), computed by se_simple_kernel.  status[i] = 1: the read is decided and ends in one record —
 * desc[i].req = 0 and req[i] describe its line (flag without the strand bit), or desc[i].req = -3: the unmapped record (flag 4, no
 * request).  Any other value: the kernel leaves the read to the library's host path; the value names the test that said so
 * (0 not looked at, 2 comment column, 3 more than mi355x_pair_maxreg() regions, 4 two regions to patch, 5 region longer than the
 * per-length table, 6 region on an ALT contig, 10 second primary region: supplementary line, 11 a secondary region with an XA entry).
 * Returns 0. */
int mi355x_se_batch(const mem_opt_t *opt, const bntseq_t *bns, int64_t n_processed, int n_reads, const void *regs, const int *n_regs,
                    int max_len, uint8_t *status, void *desc, void *req);

/* The same decisions for the reads se_simple_kernel leaves because they carry more than mi355x_pair_maxreg() regions (code 3) or a
 * secondary region with an XA entry (code 11): se_wave_kernel, a read per wavefront, 0 .. mi355x_pair_wave_maxreg() regions.  n_work
 * reads given by their numbers in the chunk (read_no[t]: mem_mark_primary_se runs with id = n_processed + read_no[t], and req.read =
 * read_no[t]) and their regions AFTER mem_sort_dedup_patch, 64-byte records back to back (the layout of mi355x_pair_wave_batch), work
 * item t owns regs[reg_off[t] .. reg_off[t+1]): there is neither a redundancy pass nor a patch alignment on the device.  Everything
 * comes back by work item.  status[t] = 1: decided with a plain record, desc[t] / req[t] as mi355x_se_batch returns them (desc.req = -3:
 * the unmapped record, no request); 16: decided with an XA tag (mem_gen_alt, src/bwamem_extra.c:98-118: the hits i, in list order, with
 * secondary_all = the line's hit and score >= its score * XA_drop_ratio; 1 .. max_XA_hits of them) — xa_cnt[t] entries, entry j's request
 * (what mem_reg2aln would ask, its contig in `pad`) at xa_req[t * mi355x_pair_wave_xa_cap() + j], the count also in desc[t].flag bits
 * 16-19: the read's requests in a job are [req[t], its XA entries'], which is how mi355x_sam_se_batch reads a descriptor with a count.
 * Any other value: the host's read, desc[t].req = req[t].read = -1; 5 a region longer than the per-length table, 6 a region on an ALT
 * contig, 10 a second primary region (supplementary line), 11 XA entries without room for them (xa_req == NULL: the kernel runs without
 * the listing; or max_XA_hits beyond the cap), 13 more than mi355x_pair_wave_maxreg() regions, 14 two hits equal under (score, hash).
 * Returns 0. */
int mi355x_se_wave_batch(const mem_opt_t *opt, const bntseq_t *bns, int64_t n_processed, int n_work, const int *read_no, const void *regs,
                         const int *reg_off, int max_len, uint8_t *status, void *desc, void *req, uint8_t *xa_cnt, void *xa_req);

/* mi355x_se_wave_batch with the kernel's side arrays for reads whose record has several lines (mem_reg2sam, src/bwamem.c:1015-1032,
 * without MEM_F_ALL and without ALT hits: every primary region of at least T, in list order, is a line).  status[t] = 17: decided with
 * n_lines[t] = 2 .. mi355x_se_lines_cap() lines; desc[t] / req[t] / xa_cnt[t] are not written for such a read.  Line j sits in slot
 * x = t * mi355x_se_lines_cap() + j of line_desc (48-byte descriptors), line_req (40-byte requests) and line_xa_cnt: the descriptor's
 * flag is 0 for line 0, 0x800 behind it (0x100 under MEM_F_NO_MULTI, as mem_aln2sam prints 0x10000; the line is a supplementary one
 * all the same), with the line's XA count in bits 16-19; mapq is mem_approx_mapq_se of the line's own region, lowered to line 0's
 * behind it unless MEM_F_KEEP_SUPP_MAPQ (:1029); sub is the region's; every line's XA entries are mem_gen_alt's for its own region,
 * entry i's request at line_xa_req[x * mi355x_pair_wave_xa_cap() + i].  desc.req is the line's request counted from the read's first when
 * the read's requests are laid out as [line 0, its XA entries', line 1, its XA entries', ...], which is how mi355x_sam_se_lines_batch
 * reads them.  More than mi355x_se_lines_cap() lines: 10 as before; line_xa_req == NULL or max_XA_hits beyond the cap: a read with 1 ..
 * max_XA_hits entries on any line gets 11 (slots of line_xa_req may have been written for such a read; no count names them).
 * n_lines == NULL: exactly mi355x_se_wave_batch.  Returns 0. */
int mi355x_se_lines_cap(void);
int mi355x_se_wave_lines_batch(const mem_opt_t *opt, const bntseq_t *bns, int64_t n_processed, int n_work, const int *read_no, const void *regs,
                               const int *reg_off, int max_len, uint8_t *status, void *desc, void *req, uint8_t *xa_cnt, void *xa_req,
                               uint8_t *n_lines, void *line_desc, void *line_req, uint8_t *line_xa_cnt, void *line_xa_req);

/* The redundancy pass of mem_sort_dedup_patch (src/bwamem.c:437-489) on the device, on raw region lists as mem_chain2aln leaves them:
 * 64-byte records back to back (the layout of mi355x_pair_wave_batch), read r owns regs[reg_off[r] .. reg_off[r+1]).  status[r] = 1: taken
 * — m[r] regions survive and keep[reg_off[r] + k], k < m[r], is the place in the read's own list of the k-th region of the reference's
 * result (after the second sort and the removal of exact duplicates); reads with 0 or 1 regions are taken with m = n.  3: more than
 * mi355x_dedup_maxreg() regions; 4: two regions pass the cheap tests of mem_patch_reg (:411-423) and the reference would go on to its
 * global alignment — such a read is the host's, m[r] = -1 and its span of keep is not written.  keep (reg_off[n_reads] ints) is sent to
 * the device as the caller filled it and comes back as the device left it: nothing is written past k = m[r].  Returns 0. */
int mi355x_dedup_maxreg(void);
int mi355x_dedup_batch(const mem_opt_t *opt, const bntseq_t *bns, int n_reads, const void *regs, const int *reg_off, uint8_t *status, int *m,
                       int *keep, double *kernel_ms);

/* mi355x_sam_batch's twin for single-end descriptors(the single-end instantiation of sam_emit_kernel): n_reads reads, read i owns
 * reqs[req_base[i] .. req_base[i+1]) (req_base: n_reads + 1 entries) and there is no mate: RNEXT PNEXT TLEN are "* 0 0", no MC tag,
 * FLAG is desc.flag | 0x10 on the reverse strand; a read is handed back (-1) alone.  Everything else — arena, guard, cursor,
 * grid_blocks, hdr_out — as above. */
int mi355x_sam_se_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_reads, const uint8_t *reads, const int64_t *off,
                        const uint8_t *quals, const char *names, const int *name_off, const void *desc, const void *reqs, const int *req_base,
                        size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off, uint8_t *arena_out,
                        unsigned long long *cursor, void *hdr_out);

/* The text of single-end reads with several lines: aln_kernel, then sam_lines_kernel (a read per wavefront) on the descriptors of
 * mi355x_se_wave_lines_batch.  n_lines[i] = 2 .. mi355x_se_lines_cap() (0: not a read of the device's, out_len[i] = -2); desc holds
 * mi355x_se_lines_cap() descriptors per read, line j of read i at [i * cap + j]; read i owns reqs[req_base[i] .. req_base[i+1]), laid
 * out as [line 0, its XA entries', line 1, ...] with reqs.read = i.  Every line is written as mem_aln2sam (src/bwamem.c:825-946) writes
 * it for an entry of a list of n_lines: lines behind the first with H for the clips and SEQ / QUAL cut to the aligned part unless
 * MEM_F_SOFTCLIP, every line with SA:Z: naming the others (CIGAR with S, MAPQ as in the descriptors, NM), then XA:Z:.  out_len[i] = the
 * bytes of all the read's lines, which lie back to back at out_off[i]; -1: the host's read, whole (aln_kernel declined one of its
 * requests; a line's short fields beyond mi355x_sam_lines_row() bytes, what the other lines' SA tags say of a line behind its contig name
 * beyond mi355x_sam_lines_sa_stage() bytes, an XA entry beyond 64 bytes; the arena is full).  Arena, guard, cursor, grid_blocks and
 * hdr_out as for mi355x_sam_se_batch. */
int mi355x_sam_lines_row(void);
int mi355x_sam_lines_sa_stage(void);
int mi355x_sam_se_lines_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_reads, const uint8_t *reads, const int64_t *off,
                              const uint8_t *quals, const char *names, const int *name_off, const uint8_t *n_lines, const void *desc,
                              const void *reqs, const int *req_base, size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off,
                              uint8_t *arena_out, unsigned long long *cursor, void *hdr_out);

/* The text of pairs that mem_sam_pe reports end by end (no_pairing:, src/bwamem_pair.c:371-392): aln_kernel, then the paired
 * instantiation of sam_lines_kernel (a pair per wavefront) on the descriptors of mi355x_pair_wave_lines_batch.  Every pair is a unit;
 * n_lines[2k + e] = 0 .. mi355x_se_lines_cap() lines of end e, desc holds mi355x_se_lines_cap() descriptors per read, line j of read r
 * at [r * cap + j]; pair k owns reqs[req_base[k] .. req_base[k+1]), laid out as [end 0: line 0, its XA entries', line 1, ...; end 1:
 * ...] with reqs.read = 2k + e.  Every line is written as mem_aln2sam writes it with a mate (src/bwamem.c:830-840, 856-867, 908): the
 * mate of every line of end e is line 0 of the other end.  An end without a line is the unaligned record: with an aligned mate it takes
 * the mate's contig, position and strand (flag 0x4, CIGAR *, RNEXT =, TLEN 0, MC:Z:, AS:i:0 XS:i:0), without one the columns are
 * "* 0 0 * * 0 0".  A line whose mate is unaligned prints its own position as PNEXT, flag 0x8, TLEN 0, no MC.  On lines behind the first,
 * and not under MEM_F_SOFTCLIP, MC:Z: prints the mate's clips as H.  An end of one line has no SA tag.  Tags: NM MD MC AS XS RG SA XA.
 * out_len[r] = the bytes of all lines of read r at out_off[r]; -1: the host's pair, both reads (the reasons of
 * mi355x_sam_se_lines_batch, on any line of either end).  Arena, guard, cursor, grid_blocks and hdr_out as for mi355x_sam_batch. */
int mi355x_sam_pe_lines_batch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int n_pairs, const uint8_t *reads, const int64_t *off,
                              const uint8_t *quals, const char *names, const int *name_off, const uint8_t *n_lines, const void *desc,
                              const void *reqs, const int *req_base, size_t arena_bytes, int grid_blocks, int *out_len, unsigned long long *out_off,
                              uint8_t *arena_out, unsigned long long *cursor, void *hdr_out);

/* Seed enumeration between SMEM and SA lookup (src/bwamem.c:161, 265-283): seed_prep_kernel (sort of a read's intervals by info,
 * l_rep, number of seeds), the prefix sum over the counts, seed_enum_kernel (BWT row and (qbeg, len) of every seed, stepping through
 * intervals larger than max_occ).  Read r has n_intv[r] intervals (x0, x1, size, info) from intv[4 * cap * r], in any order; with
 * n_intv[r] > cap the first cap count.  intv comes back sorted; read r's seeds are rows / qbeg_len (2 ints per seed) from
 * seed_off[r] (n_reads + 1 entries).  Returns the number of seeds, or -1 - that number when it exceeds seed_cap (rows and qbeg_len
 * are then not written). */
int64_t mi355x_seed_batch(int n_reads, int cap, int max_occ, uint64_t *intv, const int *n_intv, int *n_seeds, int *l_rep,
                          int64_t *seed_off, uint64_t *rows, int32_t *qbeg_len, int64_t seed_cap);

/* Mate-rescue local alignment: ksw_align2() exactly as mem_matesw() calls it (src/bwamem_pair.c:150-177,
 * src/ksw.c:321-356), for n_req windows [rb,re) of a 2-bit packed reference (doubled coordinate) against reads
 * given as nt4 codes (read r = reads[off[r]..off[r+1]) ).  out8 per request: score, te, qe, score2, te2, tb, qb
 * (kswr_t, src/ksw.h:14-20) and flags (1 = the device declined, recompute on the host). */
int mi355x_matesw_batch(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, int n_reads, const uint8_t *reads,
                        const int64_t *off, int n_req, const int64_t *rb, const int64_t *re, const int *read,
                        const int *is_rev, int *out8, double *kernel_ms);
/* Of the last mi355x_matesw_batch: what the second pass (b[] scan and reverse pass) ran — quads of two alignments of one class,
 * quads of one (the odd last member of a class), work items of a register launch, work items of the general launch. */
void mi355x_matesw_batch_counts(uint64_t out[4]);

/* ---- the caller's side of the boundary: FASTQ text -> mpiBWA's chunks -> bseq1_t[] ----
 * Record scan (find_reads_size_and_offsets, src/parallel_aux.c:682-832): offsets of the record starts
 * (rec_off[n] = end of data) and bases per record; returns the number of records or -(position+1) of a malformed one. */
int64_t mi355x_fastq_scan(const char *buf, int64_t len, int64_t cap, int64_t *rec_off, int32_t *rec_bases);
/* Chunk rule (find_chunks_info, src/parallel_aux.c:1510-1546): a chunk takes records until its base count EXCEEDS
 * maxsiz (= K/2 per file for equal-size pairs, src/mainParallel.c:947; K over both files for trimmed pairs, :1874,
 * pass bases2; K for single-end, :2773).  chunk_first[c] = first record of chunk c, chunk_first[n_chunks] = n. */
int64_t mi355x_fastq_chunks(const int32_t *bases1, const int32_t *bases2, int64_t n, int64_t maxsiz, int64_t cap,
                            int64_t *chunk_first);
/* bseq1_t[] of records [first, first+count) as mpiBWA's main builds them (src/mainParallel.c:1257-1301, :2271-2345):
 * strings NUL-terminated in place inside buf1 / buf2, mates interleaved, name cut at the first white space and a
 * trailing "/digit" dropped.  lockstep: equal-size mode (R2 cut at R1's offsets).  Returns the bases of the chunk. */
int64_t mi355x_fastq_fill(char *buf1, const int64_t *off1, char *buf2, const int64_t *off2, int64_t first, int64_t count,
                          int copy_comment, int lockstep, bseq1_t *seqs);

/* timing of the calling thread's last mem_process_seqs() call (of the last call of any thread when this thread
 * has made none), per stage (ms) */
typedef struct {
	double total_ms, h2d_ms, smem_ms, sa_ms, chain_ms, ext_ms, regs_ms, pestat_ms, sam_ms;
	double k_smem_ms, k_sa_ms, k_ext_ms;        /* HIP-event kernel times */
	uint64_t smem_bytes, sa_bytes, ext_cells;    /* algorithmic work counted on device */
	uint64_t n_reads, n_intv, n_seeds, n_chains, n_ext;
	double plan_ms, aln_ms, k_aln_ms;            /* SAM stage: decisions+collect, CIGAR kernel round trip, its HIP-event time */
	uint64_t n_aln;
	double phase1_ms;                            /* wall time of stages 2-6 (sub-batches overlap, so it is less than their sum) */
	double msw_ms, k_msw_ms;                     /* mate rescue: listing the alignments + waiting for them, HIP-event kernel time */
	uint64_t n_msw;                              /* local alignments computed by the mate-rescue kernel */
	double emit_ms;                              /* SAM stage: the pass that formats the records */
	uint64_t n_sub;                              /* sub-batches of the chunk = launches of each phase-1 kernel */
	uint64_t smem_tab_bytes;                     /* the part of smem_bytes (64 B per occ block) that the third pass took from its jump table instead of fetching */
	uint64_t n_sam_dev;                          /* SAM records written by sam_kernel (the rest are formatted by the host) */
	uint64_t n_pair_dev;                         /* pairs whose pairing decisions (mem_sam_pe) were taken on the device (pair_kernel.hip) */
	uint64_t n_se_dev;                           /* single-end reads decided on the device with a plain record, by either kernel (se_kernel.hip, se_wave_kernel.hip); their records count in n_sam_dev */
	uint64_t n_pair_wave_dev;                    /* pairs with mate rescue or up to 64 hits per end decided on the device (pair_wave_kernel.hip); not counted in n_pair_dev */
	uint64_t n_pair_xa_dev;                      /* pairs pair_wave_kernel decided because its XA listing is on: with an XA tag on a record, or left by pair_kernel.hip for its XA test alone and found to carry none; counted in neither of the two above */
	uint64_t n_dedup_dev;                        /* reads with two or more raw regions whose mem_sort_dedup_patch result was taken from the device (dedup_kernel.hip, MPIBWA_DEV_DEDUP=1) */
	uint64_t n_dedup_host;                       /* ... and those the host sorted (all of them unless MPIBWA_DEV_DEDUP=1 enables the stage; then the ones the kernel declined) */
	uint64_t n_se_wave_dev;                      /* the part of n_se_dev decided by se_wave_kernel (se_wave_kernel.hip): reads se_simple_kernel left for more than eight regions or for its XA test, whose record is plain */
	uint64_t n_se_xa_dev;                        /* single-end reads se_wave_kernel decided with an XA tag on the record; counted neither in n_se_dev nor, their records, in n_sam_dev */
	uint64_t n_se_xa_sam_dev;                    /* ... and how many of those records sam_kernel wrote (the rest came back and were aligned and formatted by the host) */
	uint64_t n_se_supp_dev;                      /* single-end reads se_wave_kernel decided with more than one line (a primary and supplementary lines with SA tags); counted in none of n_se_dev, n_se_wave_dev, n_se_xa_dev, nor, their records, in n_sam_dev */
	uint64_t n_se_supp_sam_dev;                  /* ... and how many of those reads' text sam_lines_kernel wrote (the rest came back and were aligned and formatted by the host) */
	uint64_t n_pair_lines_dev;                   /* pairs that mem_sam_pe reports end by end (no_pairing:) decided by pair_wave_kernel with 0 to 4 lines per end (MPIBWA_HOST_PAIR_LINES=1: off); counted in none of n_pair_dev, n_pair_wave_dev, n_pair_xa_dev, nor, their records, in n_sam_dev */
	uint64_t n_pair_lines_sam_dev;               /* ... and how many of those pairs' text sam_lines_kernel wrote (the rest came back and were decided, aligned and formatted by the host) */
} mi355x_stats_t;
void mi355x_last_stats(mi355x_stats_t *st);

/* host-logic test hook (no GPU involved): ksw_align2 (src/ksw.c:343-365) as used by mate rescue;
 * out7 = score,te,qe,score2,te2,tb,qb; portable != 0 runs the lane-by-lane statement instead of SSE2 */
void mi355x_host_ksw_align2(int qlen, const uint8_t *query, int tlen, const uint8_t *target, const int8_t *mat, int o_del,
                            int e_del, int o_ins, int e_ins, int xtra, int portable, int out7[7]);

/* host-logic test hook (no GPU involved): mem_sam_pe (src/bwamem_pair.c:250-393) as the library's host path runs it — the path of the
 * pairs the pairing kernel leaves to the host: rescue loop, more than eight hits per end, XA, supplementary lines — on the regions of the
 * two ends given as the reference's own mem_alnreg_t records (88 bytes each, src/bwamem.h:59-77; what mem_align1_core returns).
 * s[k].seq: nt4 codes; s[k].sam is set.  Returns the number of rescued hits. */
int   mi355x_host_sam_pe(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, const mem_pestat_t pes[4], uint64_t id, bseq1_t s[2],
                         const void *regs0, int n0, const void *regs1, int n1);
/* the same kind of hook for mem_sort_dedup_patch (src/bwamem.c:437-489; the regions of one read as mem_chain2aln leaves them, kept ones
 * written back in their new order, their number returned; query: nt4 codes) and for the single-end half of worker2 (src/bwamem.c:
 * 1187-1203: mem_mark_primary_se with id, mem_reorder_primary5 under -5, mem_reg2sam; s->sam is set) */
int   mi355x_host_sort_dedup_patch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, uint8_t *query, void *regs, int n);
void  mi355x_host_reg2sam_se(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, bseq1_t *s, const void *regs, int n, int64_t id);
/* ... and for mem_pestat (src/bwamem_pair.c:46-109): regs = the regions of n reads (mates interleaved) one after the other, n_regs[i] of read i */
void  mi355x_host_pestat(const mem_opt_t *opt, int64_t l_pac, int n, const void *regs, const int *n_regs, mem_pestat_t pes[4], int n_threads);
/* ... and for mem_flt_chained_seeds / mem_seed_sw (src/bwamem.c:571-617; reads of ~700 bp and more): the chains of a read by their seeds
 * (mem_seed_t records of 24 bytes, n_seeds[c] per chain, chain after chain); the kept seeds are written back at the start of every chain's
 * slot with their scores, n_seeds[c] updated */
void  mi355x_host_flt_chained_seeds(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, int l_query, const uint8_t *query, int n_chains,
                                    void *seeds, int *n_seeds);

/* CPUs usable by this process (cgroup quota aware) — what the host stages are sized to. */
int   mi355x_host_cpus(void);
/* Caller-side convenience equal to mpiBWA's copy_buffer_thr (src/mainParallel.c:103-127): concatenates
 * every seqs[i].sam into one malloc()ed buffer (returned, NUL-terminated, *total_len bytes) and free()s
 * the per-read strings. */
char *mi355x_collect_sam(bseq1_t *seqs, int n, size_t *total_len);
/* the same into a buffer the caller keeps from chunk to chunk (*buf / *cap: replaced when a chunk needs more); returns the length */
size_t mi355x_collect_sam_into(bseq1_t *seqs, int n, char **buf, size_t *cap);

/* ---- the caller's side behind the call: what mpiBWA does with a chunk's SAM text before it reaches the file ----
 * -f fixmate (fixmate(), src/fixmate.c:601-827): the lines of a pair get the mate's contig / position / strand, MQ, MC and ms tags;
 * seqs[2p].sam / seqs[2p+1].sam are replaced (malloc family).  mi355x_fixmate_pair: one pair, returns its number of SAM lines or -1
 * when the text is not a pair's (left untouched); mi355x_fixmate: the pairs of a chunk on the rank's host threads (call_fixmate,
 * src/parallel_aux.c:2164-2206), returns the lines or -(first read of a failing pair) - 1. */
int     mi355x_fixmate_pair(bseq1_t *s1, bseq1_t *s2, const bntseq_t *bns);
int64_t mi355x_fixmate(bseq1_t *seqs, int n, const bntseq_t *bns);
/* -g / -b output (deflate_block, src/bgzf.c:245-330; compress_and_write_bgzf_thread / _bam_thread, src/parallel_aux.c:2941-3176):
 * SAM text as BGZF blocks of whole records, compressed side by side, byte-identical for any thread count.  out needs
 * mi355x_bgzf_bound(len) bytes; returns the compressed size (0: cap too small).  mi355x_bgzf_eof: the 28-byte empty block the
 * reference appends to its .bam (src/mainParallel.c:1509-1516). */
size_t  mi355x_bgzf_bound(size_t len);
size_t  mi355x_bgzf_compress(const char *text, size_t len, int level, uint8_t *out, size_t cap);
size_t  mi355x_bgzf_eof(uint8_t out[28]);
/* The same blocks made on the device: the cuts and the contract of mi355x_bgzf_compress — out needs mi355x_bgzf_bound(len)
 * bytes, returns the compressed size, 0 when cap is too small or len is 0 — with the device encoder's one setting instead of a level
 * (LZ77 matches and dynamic Huffman codes, stored blocks where they are smaller).  The same text gives the same bytes on every call.
 * Needs a usable MI355X, no CPU fallback; re-entrant, also beside mem_process_seqs calls in flight; mi355x_finalize() gives its
 * buffers back.  mi355x_bgzf_dev_counts: blocks, blocks written stored, bytes of text, bytes of blocks — since load, all callers. */
size_t  mi355x_bgzf_compress_dev(const char *text, size_t len, uint8_t *out, size_t cap);
void    mi355x_bgzf_dev_counts(uint64_t out[4]);
/* BGZF input.  A BGZF file is a chain of independent gzip members of at most 64 KiB, each with its size in the header
 * (BSIZE) and its text's size in the trailer (ISIZE), so a file can be entered anywhere and its blocks inflated side by side.
 * mi355x_bgzf_find_block: the first offset of buf at which a block starts — a header (1f 8b 08 04 .. XLEN 6, 'B' 'C' 02 00, BSIZE) from
 * which the BSIZE hops meet two more headers or, with at_eof, the end of buf exactly; -1 when there is none, -2 when more bytes are
 * needed to decide.  mi355x_bgzf_scan: the headers from offset 0, at most cap blocks: blk_off[i] = start of block i, blk_off[n] = end of
 * the last whole block, text_off[i] = sum of the ISIZEs before block i (arrays of cap + 1); returns n, or -(offset) - 1 of a header that
 * is not one.  mi355x_bgzf_inflate: whole blocks to their text in out[cap] by zlib on the rank's host threads, every block's CRC32 and
 * ISIZE checked; returns the text's size, -(offset of the first failing block) - 1, or 0 with nothing written when cap is too small.
 * mi355x_bgzf_inflate_dev: the same results from the device decoder (one wavefront per block).  Needs a usable MI355X, no CPU
 * fallback; re-entrant, with or without a resident index, also beside mem_process_seqs and mi355x_bgzf_compress_dev calls in flight;
 * mi355x_finalize() gives its buffers back.  mi355x_bgzf_inflate_dev_counts: blocks, blocks that failed, compressed bytes, text bytes
 * — since load, all callers. */
int64_t mi355x_bgzf_find_block(const uint8_t *buf, int64_t len, int at_eof);
int64_t mi355x_bgzf_scan(const uint8_t *buf, int64_t len, int64_t cap, int64_t *blk_off, int64_t *text_off);
int64_t mi355x_bgzf_inflate(const uint8_t *in, size_t len, char *out, size_t cap);
int64_t mi355x_bgzf_inflate_dev(const uint8_t *in, size_t len, char *out, size_t cap);
void    mi355x_bgzf_inflate_dev_counts(uint64_t out[4]);
/* mpiBWAByChr's routing (src/mainParallelByChromosome.c:1340-1455, :3437-3486): the records of `sam` by destination — contig
 * 0 .. n_seqs-1 by RNAME, then "discordant" (only when discordant != 0; a record whose RNAME and RNEXT are two different contigs
 * goes to its contig AND there), last "unmapped" (RNAME '*').  out_text[d] (malloc, NULL when empty) / out_len[d] for
 * d < n_seqs + 1 + (discordant != 0).  Returns the number of records or -(offset of a malformed line) - 1. */
int64_t mi355x_route_by_chr(const char *sam, size_t len, const bntseq_t *bns, int discordant, char **out_text, size_t *out_len);
/* BAM output: a chunk's SAM text as BAM records — int32 block_size, the 32-byte core (refID, pos, l_read_name, mapq, bin,
 * n_cigar_op, flag, l_seq, next_refID, next_pos, tlen), QNAME NUL, CIGAR words, SEQ nibbles, QUAL - 33, tags in the smallest type that
 * holds them (csrc/bam_util.h states the layout once for host and device).  All return a size, 0 with nothing written when cap is too
 * small, or -(offset of the first malformed line) - 1: fewer than 11 fields, an RNAME / RNEXT that bns does not have, a non-digit in a
 * number, QUAL of another length than SEQ, a last line without '\n', a value no BAM record holds.
 * mi355x_bam_header: "BAM\1", l_text, the SAM header text, n_ref and bns's contigs (name, length).  Host only.
 * mi355x_bam_bound: room for the records of sam_len bytes of SAM text.
 * mi355x_sam_to_bam: the records back to back, on the rank's host threads; *n_records (may be NULL) = their number.
 * mi355x_bam_compress: the records as BGZF blocks at zlib's level, a block holds as many whole records as fit 0xff00 bytes; out of
 * mi355x_bgzf_bound(mi355x_bam_bound(len)) bytes always suffices.
 * mi355x_sam_to_bam_dev / mi355x_bam_compress_dev: the same records from the device encoder (csrc/bam_kernel.hip), the latter through
 * the device deflate of mi355x_bgzf_compress_dev, with that call's contract: needs a usable MI355X, no CPU fallback for a missing GPU;
 * re-entrant, also beside mem_process_seqs calls in flight; the same text gives the same bytes on every call; mi355x_finalize() gives
 * the buffers back.  A piece of text with a line the device declines ('B' tags, floats with an exponent, records above 0xff00 bytes) is
 * encoded by the host encoder: the records are the same bytes.
 * mi355x_bam_dev_counts: records, records encoded by the host because the device declined their piece, SAM bytes, BAM bytes, blocks,
 * compressed bytes — since load, all callers. */
int64_t mi355x_bam_header(const char *text, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap);
int64_t mi355x_bam_bound(size_t sam_len);
int64_t mi355x_sam_to_bam(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap, int64_t *n_records);
int64_t mi355x_sam_to_bam_dev(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap, int64_t *n_records);
int64_t mi355x_bam_compress(const char *sam, size_t len, const bntseq_t *bns, int level, uint8_t *out, size_t cap);
int64_t mi355x_bam_compress_dev(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap);
void    mi355x_bam_dev_counts(uint64_t out[6]);
/* Coordinate-sorted BAM: a complete BAM file in memory (BGZF blocks, with or without the empty end block) to a complete
 * BAM file in samtools' coordinate order — refID (-1 behind every contig), pos + 1, the reverse-strand bit, ties in input order; the
 * @HD line of the header text says SO:coordinate (csrc/bam_sort_util.h states the hop, the validation, the key and the header rule once
 * for host and device).  The header goes out in BGZF blocks of its own, the records in blocks of whole records of at most 0xff00 bytes
 * (a larger record alone, cut into such blocks), then the 28-byte empty block.
 * mi355x_bam_sort_bound: the bytes out needs, from the blocks' ISIZEs; -(offset) - 1 for a file whose blocks do not scan.
 * mi355x_bam_sort: on the rank's host threads (MPIBWA_SAMPOST_THREADS), zlib at `level`.  Returns the size written; 0 with nothing
 * written when cap is below mi355x_bam_sort_bound(bam, len); -(offset) - 1 for input that is not a BAM file or fails validation, where
 * the offset is an INPUT FILE offset for a bad BGZF block (a header that is none, a block the file cuts off, a failed inflate, CRC or
 * ISIZE) and an offset into the INFLATED STREAM for a bad header (the magic: 0) or record (block_size < 32, a record that runs past the
 * end, refID < -1 or >= n_ref, pos < -1).  Bad blocks are reported before bad records.
 * mi355x_bam_sort_dev: the same from the device — inflate, record walk, radix sort, record gather and deflate kernels: the same return
 * codes, the same record stream and cuts (every block inflates to the bytes of the host path's block of the same number), the device
 * deflate's one setting, the same bytes on every call.  Needs a usable MI355X, no CPU fallback for a missing GPU; re-entrant (one sort
 * holds the device's sort buffers at a time, other callers wait), also beside mem_process_seqs calls in flight; mi355x_finalize() gives
 * the buffers back.  INT64_MIN with nothing written: the file does not fit the device's free memory (the inflated stream, 40 bytes a
 * record and about 0.4 GB of fixed buffers, less a margin of 256 MiB; MPIBWA_BAM_SORT_MAX_BYTES=<bytes> caps what is admitted).
 * mi355x_bam_sort_dev_counts: calls, records, calls whose record walk the host did (a foreign writer's blocks: records that span
 * blocks), inflated bytes, input blocks, output blocks, compressed bytes out, calls refused for memory — since load, all callers.
 * A file of 2^31 - 2 records or more is refused in the same way (the sort's indices are 32-bit).
 * mi355x_bam_sort_dev_refused_need: the bytes of device memory, the margin included, that the last refused call needed (0: none).
 * mi355x_bam_sort_dev_stage_ms: for tools/bench_bam_sort.py — the last finished call's wall ms of inflate, walk, sort, emit and the
 * whole call, the record gather kernels' summed device ms and the bytes they moved, 0.  With MPIBWA_BAM_SORT_GATHER_ALONE set (a
 * measurement aid, slower) a call drains its other stream before every gather launch, so that those device ms are of a kernel that
 * has the device to itself. */
int64_t mi355x_bam_sort_bound(const uint8_t *bam, size_t len);
int64_t mi355x_bam_sort(const uint8_t *bam, size_t len, int level, uint8_t *out, size_t cap);
int64_t mi355x_bam_sort_dev(const uint8_t *bam, size_t len, uint8_t *out, size_t cap);
void    mi355x_bam_sort_dev_counts(uint64_t out[8]);
void    mi355x_bam_sort_dev_stage_ms(double out[8]);
uint64_t mi355x_bam_sort_dev_refused_need(void);
/* BAI index of a coordinate-sorted BAM file (SAM specification §5.2): the file a variant caller, a viewer or a duplicate
 * marker opens the BAM file through.  csrc/bam_index_util.h states once what it contains: per record refID, pos, flag, l_read_name,
 * n_cigar_op and the CIGAR words are read (the stored bin is not); beg = max(pos, 0), end = beg + the reference bases of M, D, N, = and X
 * (1 for flag 0x4, no CIGAR or none of these), bin = reg2bin(beg, end); a maximal run of records of one bin is a chunk, chunks of a bin
 * are joined only where the second begins in the BGZF block in which the first ends (htslib's folding of small bins into their parents
 * is not done), pseudo-bin 37450 holds the contig's span and its mapped and unmapped counts, the linear index has a window per 16 384
 * positions up to the contig's last covered one, refID -1 is counted in n_no_coor.
 * mi355x_bam_index: on the rank's host threads, for any coordinate-sorted BAM file in memory, the library's own or a foreign writer's
 * (records that span blocks, empty blocks, with or without the empty end block).  *bai is malloc'ed (the caller frees it), *bai_len its
 * size.  Returns the number of records, or -(offset) - 1 with nothing allocated: bad BGZF blocks first, by INPUT FILE offset; then the
 * first record in stream order that is malformed (mi355x_bam_sort's rules), sorts before its predecessor or ends beyond 2^29, by its
 * offset in the INFLATED STREAM.  *reason (may be NULL): 0 fine, 1 a BGZF block, 2 the header or a record, 3 not in coordinate order,
 * 4 beyond 2^29 (BAI's limit).
 * mi355x_bam_index_dev: the same bytes and codes from the device — the sort's inflate kernel and record walk, then the index kernels
 * (csrc/bam_index_kernel.hip).  A file whose blocks do not end on record boundaries, or in which the device finds a malformed,
 * out-of-order or too long record, is indexed by the host path (it decides the code).  INT64_MIN: the file does not fit, under the
 * sort's admission rule (the inflated stream, 20 + 52 bytes a record, 40 a run, 8 a window).  Shares the sort's buffers and mutex.
 * mi355x_bam_sort_index_dev: mi355x_bam_sort_dev and the index of what it writes in one call — out gets exactly the bytes of
 * mi355x_bam_sort_dev, the return value and codes are the sort's, *bai is the index of out, built from the order, the cuts and the
 * compressed block sizes the sort holds on the device.  A record beyond 2^29 fails the call with reason 4 and -(its offset in the
 * input's inflated stream) - 1, nothing written.  *bai is set only when the return value is positive.
 * mi355x_bam_index_dev_counts: calls of both device entry points, records, calls whose walk the host did, runs before the join, chunks
 * written, linear windows, BAI bytes, calls refused for memory — since load, all callers.
 * mi355x_bam_index_dev_stage_ms: for tools/bench_bam_index.py — the last finished call's wall ms of inflate, walk, the index stages,
 * the serialisation and the whole call, the index kernels' summed device ms, 0, 0. */
int64_t mi355x_bam_index(const uint8_t *bam, size_t len, uint8_t **bai, size_t *bai_len, int *reason);
int64_t mi355x_bam_index_dev(const uint8_t *bam, size_t len, uint8_t **bai, size_t *bai_len, int *reason);
int64_t mi355x_bam_sort_index_dev(const uint8_t *bam, size_t len, uint8_t *out, size_t cap, uint8_t **bai, size_t *bai_len, int *reason);
void    mi355x_bam_index_dev_counts(uint64_t out[8]);
void    mi355x_bam_index_dev_stage_ms(double out[8]);

#ifdef __cplusplus
}
#endif
#endif
