// ctx_pool_check.cpp — csrc/ctx_pool.h on the host with a mock context (tests/test_ctx_pool_host.py builds and runs it; with the thread
// sanitizer every plain field below is also a race detector: the pool's protocol alone orders the accesses to a context).
//   ctx_pool_check crowd | prefer | release | init
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "ctx_pool.h"

#define CHECK(x)                                                               \
	do {                                                                       \
		if (!(x)) {                                                            \
			fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #x); \
			fflush(stderr);                                                    \
			std::_Exit(1);                                                     \
		}                                                                      \
	} while (0)

namespace {

struct Mock;
std::vector<Mock *> g_all;              // the pool's contexts in its order (they are constructed in it)
std::atomic<int> g_in_init{0};          // threads inside an init() right now
std::atomic<bool> g_meet_in_init{false};   // `init`: an init() returns only once a second one runs beside it

struct Mock {
	std::atomic<int> inside{0};         // callers of init / release / drain / work right now: never two
	std::atomic<bool> held{false};      // from the lease's first use to its drain()
	bool inited = false;                // plain, like the counts: whoever is inside owns them
	long n_init = 0, n_release = 0, n_drain = 0, n_work = 0;
	Mock() { g_all.push_back(this); }
	struct Alone {
		Mock &m;
		explicit Alone(Mock &m_) : m(m_) { CHECK(m.inside.fetch_add(1) == 0); }
		~Alone() { CHECK(m.inside.fetch_sub(1) == 1); }
	};
	void init()
	{
		Alone a(*this);
		CHECK(!held.load() && !inited);
		g_in_init.fetch_add(1);
		if (g_meet_in_init.load()) {
			const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(20);
			while (g_in_init.load() < 2) {
				CHECK(std::chrono::steady_clock::now() < until);   // the other first lease never got into its init(): init() runs under the lock
				std::this_thread::yield();
			}
		} else
			g_in_init.fetch_sub(1);
		inited = true;
		++n_init;
	}
	void release()
	{
		Alone a(*this);
		CHECK(!held.load() && inited);
		inited = false;
		std::this_thread::yield();   // (room for a lease that would take a context whose buffers are going)
		++n_release;
	}
	void drain()
	{
		Alone a(*this);
		CHECK(inited && held.load());
		++n_drain;
		held.store(false);
	}
	void work()   // what a call does with its lease
	{
		CHECK(!held.exchange(true));
		Alone a(*this);
		CHECK(inited);
		++n_work;
	}
	void consistent() const { CHECK(!held.load() && inside.load() == 0 && n_init - n_release == (inited ? 1 : 0) && n_drain == n_work); }
};

constexpr int N = 4;
using Pool = mbw::CtxPool<Mock, N>;

long total(long Mock::*f)
{
	long n = 0;
	for (Mock *m : g_all) n += m->*f;
	return n;
}

// 12 threads over 4 contexts (and a thread that releases the idle ones meanwhile, with_release): nobody shares a context, everybody is served
void crowd(bool with_release)
{
	static Pool pool;
	constexpr int THREADS = 12, LEASES = 3000;
	std::atomic<bool> done{false};
	std::vector<std::thread> t;
	for (int k = 0; k < THREADS; ++k)
		t.emplace_back([&] {
			for (int i = 0; i < LEASES; ++i) {
				Pool::Lease lease(pool);
				(*lease).work();
				if (i % 64 == 0) std::this_thread::yield();
			}
		});
	std::thread rel;
	if (with_release)
		rel = std::thread([&] {
			while (!done.load()) { pool.release_idle(); std::this_thread::yield(); }
		});
	for (std::thread &x : t) x.join();
	done.store(true);
	if (with_release) rel.join();
	for (Mock *m : g_all) m->consistent();   // ready or released, never half-done
	CHECK(total(&Mock::n_work) == (long)THREADS * LEASES && total(&Mock::n_drain) == (long)THREADS * LEASES);
	if (!with_release) {
		CHECK(total(&Mock::n_init) >= 1 && total(&Mock::n_init) <= N && total(&Mock::n_release) == 0);   // a context is initialised once
		return;
	}
	CHECK(total(&Mock::n_release) > 0);
	pool.release_idle();
	for (Mock *m : g_all) { m->consistent(); CHECK(!m->inited); }
	const long inits = total(&Mock::n_init);
	{   // leases taken afterwards initialise again
		Pool::Lease a(pool), b(pool), c(pool), d(pool);
		(*a).work(); (*b).work(); (*c).work(); (*d).work();
		CHECK(total(&Mock::n_init) == inits + N);
	}
	for (Mock *m : g_all) { m->consistent(); CHECK(m->inited); }
}

// a lease takes a context that has its buffers before one that has not, wherever they stand
void prefer()
{
	static Pool pool;
	auto take = [&] {
		Pool::Lease *l = new Pool::Lease(pool);
		(**l).work();
		return l;
	};
	Pool::Lease *a = take(), *b = take();   // contexts 0 and 1, both initialised now
	CHECK(&**a == g_all[0] && &**b == g_all[1] && total(&Mock::n_init) == 2);
	delete a;
	pool.release_idle();                    // 0 goes; 1 is held and stays
	delete b;
	CHECK(!g_all[0]->inited && g_all[0]->n_release == 1 && g_all[1]->inited && g_all[1]->n_release == 0);
	Pool::Lease *c = take();                // 1: it is ready, though 0 stands before it; nothing is initialised
	CHECK(&**c == g_all[1] && total(&Mock::n_init) == 2);
	Pool::Lease *d = take();                // no ready one is left: the first idle one, initialised now
	CHECK(&**d == g_all[0] && total(&Mock::n_init) == 3);
	delete c;
	delete d;
	for (Mock *m : g_all) m->consistent();
}

// two first leases initialise side by side: each init() waits for the other one to be inside its own
void init_outside_the_lock()
{
	static Pool pool;
	g_meet_in_init.store(true);
	std::thread a([&] { Pool::Lease l(pool); (*l).work(); }), b([&] { Pool::Lease l(pool); (*l).work(); });
	a.join();
	b.join();
	CHECK(g_in_init.load() == 2 && total(&Mock::n_init) == 2);
	for (Mock *m : g_all) m->consistent();
}

} // namespace

int main(int argc, char **argv)
{
	const char *what = argc > 1 ? argv[1] : "";
	if (!strcmp(what, "crowd")) crowd(false);
	else if (!strcmp(what, "release")) crowd(true);
	else if (!strcmp(what, "prefer")) prefer();
	else if (!strcmp(what, "init")) init_outside_the_lock();
	else { fprintf(stderr, "usage: ctx_pool_check crowd | prefer | release | init\n"); return 2; }
	CHECK((int)g_all.size() == N);
	printf("ok %s\n", what);
	return 0;
}
