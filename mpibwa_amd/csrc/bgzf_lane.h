// bgzf_lane.h — what one stream of an output-format stage needs to take a piece of at most LANE_BLOCKS blocks through the deflate kernels
// (DeflateLane: bgzf_stage.hip, bam_stage.hip, bam_sort_stage.hip) or through the inflate kernel (InflateLane: bgzf_in_stage.hip,
// bam_sort_stage.hip): the device and page-locked buffers, of one size whatever the input, and the sequence queued on the stream.  A context
// holds two lanes of a kind, one per stream; the stream, the piece's input or destination and every synchronisation stay with the stage.
// DESIGN §8.2.  (.hip files only)
#ifndef MBW_BGZF_LANE_H
#define MBW_BGZF_LANE_H
#include <array>
#include <cstring>
#include "hip_util.h"
#include "device.h"

namespace mbw {

constexpr int LANE_BLOCKS = BAM_DEV_BLOCKS;                          // blocks per piece = workgroups per launch
constexpr size_t LANE_SLOT_BYTES = 0x10000, LANE_BYTES = LANE_BLOCKS * LANE_SLOT_BYTES;   // a block, and a piece's blocks, at their largest
constexpr size_t LANE_TEXT_BYTES = (size_t)LANE_BLOCKS * BGZF_DEV_INPUT, LANE_SLACK = 16;   // what a piece deflates, and the slack behind it
constexpr size_t LANE_META_BYTES = 2 * sizeof(unsigned long long);   // d_meta: the packed bytes, the blocks written stored

// (hidden: header-only code, no symbol of a lane leaves the library)
struct __attribute__((visibility("hidden"))) DeflateLane {
	DevBuf d_cut, d_slots, d_sizes, d_out, d_meta, d_tokens;   // (tokens per lane: the two pieces' kernels may run side by side)
	PinBuf h_cut, h_out, h_meta, h_sizes;                      // h_sizes: only once want_sizes() has asked for it
	std::array<DevBuf *, 6> dev() { return {&d_cut, &d_slots, &d_sizes, &d_out, &d_meta, &d_tokens}; }
	static constexpr size_t dev_size(int i)   // of dev()[i]: the one table that init() allocates from and dev_bytes() sums
	{
		constexpr size_t bytes[6] = {sizeof(uint32_t) * (LANE_BLOCKS + 1), LANE_BYTES, sizeof(uint32_t) * LANE_BLOCKS, LANE_BYTES, LANE_META_BYTES,
		                             sizeof(uint16_t) * LANE_TEXT_BYTES};
		return bytes[i];
	}
	static constexpr size_t dev_bytes()
	{
		size_t n = 0;
		for (int i = 0; i < 6; ++i) n += dev_size(i);
		return n;
	}
	void init()
	{
		for (int i = 0; i < 6; ++i) dev()[i]->ensure(dev_size(i));
		h_cut.ensure(dev_size(0)); h_out.ensure(LANE_BYTES); h_meta.ensure(LANE_META_BYTES);
	}
	void want_sizes() { h_sizes.ensure(dev_size(2)); }
	void release()
	{
		for (DevBuf *b : dev()) b->release();
		for (PinBuf *b : {&h_cut, &h_out, &h_meta, &h_sizes}) b->release();
	}
	// the piece's cuts cut[0 .. nb], rebased to its first byte, up (the stage's own cuts; bam_stage.hip's kernels write d_cut themselves)
	template <class T> void cuts_up(hipStream_t st, const T *cut, int nb)
	{
		uint32_t *hc = (uint32_t *)h_cut.p;
		for (int k = 0; k <= nb; ++k) hc[k] = (uint32_t)(cut[k] - cut[0]);
		HIP_OK(hipMemcpyAsync(d_cut.p, hc, sizeof(uint32_t) * (nb + 1), hipMemcpyHostToDevice, st));
	}
	// d_in's nb blocks (d_in has LANE_SLACK bytes behind the last; with d_n_blocks their number is read on the device, nb = LANE_BLOCKS) to
	// complete BGZF blocks in the slots, the slots closed up into d_out, d_meta's two words back
	void queue(hipStream_t st, const uint8_t *d_in, int nb, const uint32_t *d_n_blocks = nullptr)
	{
		unsigned long long *meta = (unsigned long long *)d_meta.p;
		HIP_OK(hipMemsetAsync(meta, 0, LANE_META_BYTES, st));
		launch_bgzf_deflate(st, d_in, (const uint32_t *)d_cut.p, nb, (uint8_t *)d_slots.p, (uint32_t *)d_sizes.p, (uint16_t *)d_tokens.p, LANE_BLOCKS, meta, d_n_blocks);
		launch_bgzf_gather(st, (const uint8_t *)d_slots.p, (const uint32_t *)d_sizes.p, nb, (uint8_t *)d_out.p, meta, d_n_blocks);
		HIP_OK(hipMemcpyAsync(h_meta.p, meta, LANE_META_BYTES, hipMemcpyDeviceToHost, st));
	}
	// once the stream has run queue(): the piece's compressed bytes, and how many of its blocks were written stored
	size_t packed() const { return (size_t)((const unsigned long long *)h_meta.p)[0]; }
	uint64_t stored() const { return ((const unsigned long long *)h_meta.p)[1]; }
	// the compressed bytes' way back, queued (with n_sizes, after want_sizes(): also that many blocks' sizes, into h_sizes); once the
	// stream has run it, store() gives them to the caller
	void fetch(hipStream_t st, size_t n_sizes = 0)
	{
		HIP_OK(hipMemcpyAsync(h_out.p, d_out.p, packed(), hipMemcpyDeviceToHost, st));
		if (n_sizes) HIP_OK(hipMemcpyAsync(h_sizes.p, d_sizes.p, n_sizes * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	}
	size_t store(uint8_t *out) const
	{
		memcpy(out, h_out.p, packed());
		return packed();
	}
};

struct __attribute__((visibility("hidden"))) InflateLane {
	static constexpr size_t OFF_BYTES = sizeof(uint32_t) * 2 * (LANE_BLOCKS + 1);   // the blocks' offsets, then their texts', both rebased to the piece
	DevBuf d_comp, d_off;
	PinBuf h_comp, h_off;
	std::array<DevBuf *, 2> dev() { return {&d_comp, &d_off}; }
	static constexpr size_t dev_size(int i) { return i == 0 ? LANE_BYTES : OFF_BYTES; }   // of dev()[i], and of its page-locked twin
	static constexpr size_t dev_bytes() { return dev_size(0) + dev_size(1); }
	void init()
	{
		for (int i = 0; i < 2; ++i) dev()[i]->ensure(dev_size(i));
		h_comp.ensure(dev_size(0)); h_off.ensure(dev_size(1));
	}
	void release()
	{
		for (DevBuf *b : dev()) b->release();
		for (PinBuf *b : {&h_comp, &h_off}) b->release();
	}
	// blocks b0 .. b1 - 1 of `file` (bgzf_in_plan's blk and txt; at most LANE_BLOCKS of them) up and through the kernel: their text to d_text,
	// their status words to d_status.  The caller sees to it that the stream has done with the page-locked buffers' last load; `up`, if
	// given, is recorded behind the uploads, where this load has left them.
	void queue(hipStream_t st, const uint8_t *file, const int64_t *blk, const int64_t *txt, size_t b0, size_t b1, uint8_t *d_text, uint32_t *d_status,
	           hipEvent_t up = nullptr)
	{
		const int nb = (int)(b1 - b0);
		const size_t cbytes = (size_t)(blk[b1] - blk[b0]), tbytes = (size_t)(txt[b1] - txt[b0]);   // (each at most LANE_BYTES: a block and its text are at most 64 KiB)
		memcpy(h_comp.p, file + blk[b0], cbytes);
		uint32_t *ho = (uint32_t *)h_off.p, *hb = ho, *ht = ho + (LANE_BLOCKS + 1);
		for (int k = 0; k <= nb; ++k) { hb[k] = (uint32_t)(blk[b0 + k] - blk[b0]); ht[k] = (uint32_t)(txt[b0 + k] - txt[b0]); }
		uint32_t *dof = (uint32_t *)d_off.p;
		HIP_OK(hipMemcpyAsync(d_comp.p, h_comp.p, cbytes, hipMemcpyHostToDevice, st));
		HIP_OK(hipMemcpyAsync(dof, ho, OFF_BYTES, hipMemcpyHostToDevice, st));
		if (up) HIP_OK(hipEventRecord(up, st));
		launch_bgzf_inflate(st, (const uint8_t *)d_comp.p, (uint32_t)cbytes, dof, dof + (LANE_BLOCKS + 1), nb, d_text, (uint32_t)tbytes, d_status);
	}
};

} // namespace mbw
#endif
