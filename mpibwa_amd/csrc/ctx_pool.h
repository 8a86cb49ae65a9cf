// ctx_pool.h — the pool of call contexts behind the output-format stages (bgzf_stage.hip, bgzf_in_stage.hip, bam_stage.hip): N contexts,
// each leased to one call at a time, more callers wait their turn.  DESIGN §8.2.
//
// Ctx supplies init() (its buffers and streams), release() (all of them back) and drain() (its streams synchronised).  A context is
// initialised by the first lease that gets it and released only by release_idle(); both run OUTSIDE the pool's lock, the context being
// marked busy meanwhile, so that first calls initialise side by side and nobody waits on the lock for a hipMalloc.  `ready` is
// written only by whoever holds `busy`; the search reads it of idle contexts, under the lock.  No HIP in here:
// tests/csrc/ctx_pool_check.cpp runs it on the host with a mock context.
#ifndef MBW_CTX_POOL_H
#define MBW_CTX_POOL_H
#include <condition_variable>
#include <mutex>

namespace mbw {

template <class Ctx, int N> class CtxPool {
	struct Slot {
		Ctx ctx;
		bool busy = false, ready = false;
	};
	Slot slot_[N];
	std::mutex mu_;
	std::condition_variable cv_;

public:
	// a context for the life of the object, with its buffers
	class Lease {
		CtxPool &pool_;
		Slot *s_ = nullptr;

	public:
		explicit Lease(CtxPool &pool) : pool_(pool)
		{
			std::unique_lock<std::mutex> lk(pool_.mu_);
			for (;;) {
				for (int pass = 0; pass < 2 && !s_; ++pass)   // one that has its buffers first
					for (int i = 0; i < N && !s_; ++i)
						if (!pool_.slot_[i].busy && (pass == 1 || pool_.slot_[i].ready)) s_ = &pool_.slot_[i];
				if (s_) break;
				pool_.cv_.wait(lk);
			}
			s_->busy = true;
			lk.unlock();
			if (!s_->ready) {
				s_->ctx.init();
				s_->ready = true;
			}
		}
		// A call that ends early leaves nothing queued on the context: its streams are drained before the next call gets it.  For a
		// call that ran to its end (every call of the two BGZF stages) the streams are idle by now and this is two no-op synchronisations.
		~Lease()
		{
			s_->ctx.drain();
			{
				std::lock_guard<std::mutex> lk(pool_.mu_);
				s_->busy = false;
			}
			pool_.cv_.notify_one();
		}
		Lease(const Lease &) = delete;
		Lease &operator=(const Lease &) = delete;
		Ctx &operator*() const { return s_->ctx; }
	};

	// the buffers and streams of the contexts that no call holds (mi355x_finalize); the next lease of one initialises it again
	void release_idle()
	{
		std::unique_lock<std::mutex> lk(mu_);
		for (Slot &x : slot_) {
			if (x.busy || !x.ready) continue;
			x.busy = true;   // nobody leases it while its buffers go
			lk.unlock();
			x.ctx.release();
			x.ready = false;
			lk.lock();
			x.busy = false;
		}
		cv_.notify_all();
	}
};

} // namespace mbw
#endif
