// The executor of the HIP stand-in: memory, streams, events and the launch of a kernel on OS threads.
// Semantics: the opening comment of hip/hip_runtime.h.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <sched.h>
#include <stdlib.h>

#include <atomic>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

thread_local uint3 threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

namespace {

// Kernels that rely on the range check of a buffer resource on purpose, each with its reason.  Any other
// out-of-range buffer access aborts.  (k_extprod, the one user of buffer resources, pads its grid to whole groups of
// eight bootstraps and sizes its three resources over the padded chunk: it needs no entry.)
struct Allowed {
    const char *kernel, *reason;
};
const Allowed ALLOW_OUT_OF_RANGE[] = {{nullptr, nullptr}};

// Kernels that never run as a plain loop: they can leave every block of one launch before their first barrier.
const char *const ALWAYS_THREADED[] = {"k_circ_split"};

constexpr unsigned MAX_THREADS = 1024, WAVE = 64;
constexpr int DEFAULT_LDS_LIMIT = 64 * 1024;
constexpr int SPIN_YIELDS = 64;

[[noreturn]] void die(const char *what, const char *kernel) {
    fprintf(stderr, "hipcpu: %s (kernel %s)\n", what, kernel ? kernel : "-");
    fflush(stderr);
    abort();
}

int fill_byte() {
    static const int v = [] {
        const char *s = getenv("HIPCPU_FILL");
        return s ? (int)(strtoul(s, nullptr, 0) & 0xFF) : 0;
    }();
    return v;
}

// A barrier that threads may leave for good (a kernel thread that returned no longer counts, as on the device).
struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    unsigned expected = 0, arrived = 0, left = 0;
    std::atomic<uint64_t> gen{0};
    void reset(unsigned n) { expected = n, arrived = 0, left = 0; }
    void release() {   // under m
        arrived = 0;
        gen.fetch_add(1, std::memory_order_release);
        cv.notify_all();
    }
    template <class F>
    void wait(F &&last) {
        std::unique_lock<std::mutex> l(m);
        if (++arrived + left >= expected) {
            last();
            release();
            return;
        }
        const uint64_t g = gen.load(std::memory_order_relaxed);
        l.unlock();
        // a block's threads outnumber the cores: give the core away a few times before sleeping on the condition
        for (int i = 0; i < SPIN_YIELDS; i++) {
            if (gen.load(std::memory_order_acquire) != g) return;
            sched_yield();
        }
        l.lock();
        cv.wait(l, [&] { return gen.load(std::memory_order_acquire) != g; });
    }
    void wait() { wait([] {}); }
    void leave() {
        std::lock_guard<std::mutex> l(m);
        ++left;
        if (arrived && arrived + left >= expected) release();
    }
};

struct Wave {
    Barrier bar;
    uint64_t slot[WAVE];
    std::atomic<uint64_t> wrote{0};   // lanes that filled their slot in the exchange under way (a lane that returned has not)
    unsigned lanes = 0;
};

struct Launch {
    const char *text = nullptr;
    std::string name;
    dim3 grid, block;
    unsigned nthreads = 0;
    void (*fn)(void *) = nullptr;
    void *ctx = nullptr;
    void *lds = nullptr;
    size_t lds_bytes = 0;
    bool threaded = false;
    std::atomic<bool> synced{false};
    Barrier block_bar, end_bar;
    std::unique_ptr<Wave[]> waves;
    unsigned nwaves = 0;
};
Launch L;

struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    bool go = false, quit = false;
};
std::vector<std::unique_ptr<Worker>> pool;
std::mutex done_m;
std::condition_variable done_cv;
unsigned done_left = 0;

struct Stats {
    uint64_t launches = 0, out_of_range = 0;
};
std::map<std::string, Stats> stats;          // by kernel name
std::map<std::string, bool> plain_loop;      // by launch text: no barrier seen in the first launch
std::map<const void *, int> lds_limit;
std::mutex state_m;                          // the three maps and the error word (callers may be several threads)
std::mutex launch_m;                         // one launch at a time
thread_local hipError_t last_error = hipSuccess;

std::string kernel_name(const char *text) {
    std::string s;
    for (const char *p = text; *p; p++) {
        if (*p == '(' || *p == ' ') continue;
        if (*p == '<' || *p == ')') break;
        s += *p;
    }
    return s;
}

void prepare_block() {
    if (L.lds_bytes) memset(L.lds, fill_byte(), L.lds_bytes);
    L.block_bar.reset(L.nthreads);
    for (unsigned w = 0; w < L.nwaves; w++) L.waves[w].bar.reset(L.waves[w].lanes);
}

void set_thread(unsigned t) {
    threadIdx.x = t % L.block.x;
    threadIdx.y = (t / L.block.x) % L.block.y;
    threadIdx.z = t / (L.block.x * L.block.y);
    blockDim = L.block;
    gridDim = L.grid;
}

void run_thread(unsigned t) {
    set_thread(t);
    for (unsigned z = 0; z < L.grid.z; z++)
        for (unsigned y = 0; y < L.grid.y; y++)
            for (unsigned x = 0; x < L.grid.x; x++) {
                blockIdx.x = x, blockIdx.y = y, blockIdx.z = z;
                L.fn(L.ctx);
                L.block_bar.leave();
                L.waves[t / WAVE].bar.leave();
                L.end_bar.wait(prepare_block);
            }
}

void worker_main(Worker *w, unsigned t) {
    for (;;) {
        {
            std::unique_lock<std::mutex> l(w->m);
            w->cv.wait(l, [&] { return w->go || w->quit; });
            if (w->quit) return;
            w->go = false;
        }
        run_thread(t);
        std::lock_guard<std::mutex> l(done_m);
        if (--done_left == 0) done_cv.notify_all();
    }
}

struct PoolEnd {
    ~PoolEnd() {
        for (auto &w : pool) {
            {
                std::lock_guard<std::mutex> l(w->m);
                w->quit = true;
            }
            w->cv.notify_all();
            w->th.join();
        }
        pool.clear();
        if (const char *path = getenv("HIPCPU_LAUNCH_LOG")) {
            if (FILE *f = fopen(path, "w")) {
                for (const auto &kv : stats)
                    fprintf(f, "%s %llu %llu\n", kv.first.c_str(), (unsigned long long)kv.second.launches,
                            (unsigned long long)kv.second.out_of_range);
                fclose(f);
            }
        }
    }
} pool_end;

inline void mark_sync(const char *what) {
    if (!L.threaded) die(what, L.text);
    L.synced.store(true, std::memory_order_relaxed);
}
inline unsigned flat_tid() { return threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z); }

hipError_t fail(hipError_t e) {
    last_error = e;
    return e;
}

}  // namespace

namespace hipcpu {

void *dynamic_lds() { return L.lds; }

void syncthreads() {
    mark_sync("__syncthreads in a kernel that ran as a plain loop");
    L.block_bar.wait();
}

void wave_barrier() {
    mark_sync("wavefront fence in a kernel that ran as a plain loop");
    L.waves[flat_tid() / WAVE].bar.wait();
}

uint64_t shfl_xor64(uint64_t v, int lane_mask) {
    mark_sync("__shfl_xor in a kernel that ran as a plain loop");
    Wave &w = L.waves[flat_tid() / WAVE];
    const unsigned lane = flat_tid() % WAVE, src = lane ^ (unsigned)lane_mask;
    w.slot[lane] = v;
    w.wrote.fetch_or(1ull << lane);
    w.bar.wait();
    // a source lane that is outside the wave or has returned gives the lane its own value back
    const uint64_t r = src < w.lanes && (w.wrote.load() >> src & 1) ? w.slot[src] : v;
    w.bar.wait();
    w.wrote.fetch_and(~(1ull << lane));
    return r;
}

uint32_t readfirstlane(uint32_t v) {
    mark_sync("readfirstlane in a kernel that ran as a plain loop");
    Wave &w = L.waves[flat_tid() / WAVE];
    w.slot[flat_tid() % WAVE] = v;
    w.wrote.fetch_or(1ull << (flat_tid() % WAVE));
    w.bar.wait();
    const uint32_t first = (uint32_t)w.slot[__builtin_ctzll(w.wrote.load())];   // the first lane still running
    w.bar.wait();
    w.wrote.fetch_and(~(1ull << (flat_tid() % WAVE)));
    if (first != v) die("readfirstlane of a value that is not uniform over the wavefront", L.text);
    return first;
}

void buffer_out_of_range() {
    {
        std::lock_guard<std::mutex> l(state_m);
        stats[L.name].out_of_range++;
    }
    for (const Allowed &a : ALLOW_OUT_OF_RANGE)
        if (a.kernel && L.name == a.kernel) return;
    die("buffer-resource access out of range", L.text);
}

void launch_blocks(const char *text, const void *func, dim3 grid, dim3 block, size_t lds, void (*thread_fn)(void *),
                   void *ctx) {
    std::lock_guard<std::mutex> serial(launch_m);
    const uint64_t nthreads = (uint64_t)block.x * block.y * block.z;
    if (!nthreads || nthreads > MAX_THREADS || !grid.x || !grid.y || !grid.z) {
        fail(hipErrorInvalidConfiguration);
        return;
    }
    bool plain;
    {
        std::lock_guard<std::mutex> l(state_m);
        const auto lim = lds_limit.find(func);
        if (lds > (size_t)(lim == lds_limit.end() ? DEFAULT_LDS_LIMIT : lim->second)) {
            fail(hipErrorInvalidValue);
            return;
        }
        const auto p = plain_loop.find(text);
        plain = p != plain_loop.end() && p->second;
        L.name = kernel_name(text);
        stats[L.name].launches++;
    }
    L.text = text;
    L.grid = grid, L.block = block, L.nthreads = (unsigned)nthreads;
    L.fn = thread_fn, L.ctx = ctx;
    L.lds_bytes = lds;
    L.lds = nullptr;
    if (posix_memalign(&L.lds, 16, lds ? lds : 1) != 0) die("no memory for the dynamic LDS", text);
    // (a launch without dynamic LDS gets a block of one byte: any 32-bit access of it is out of bounds)
    L.threaded = !plain;
    L.synced = false;
    if (plain) {
        const dim3 g = grid;
        for (unsigned z = 0; z < g.z; z++)
            for (unsigned y = 0; y < g.y; y++)
                for (unsigned x = 0; x < g.x; x++) {
                    if (lds) memset(L.lds, fill_byte(), lds);
                    for (unsigned t = 0; t < L.nthreads; t++) {
                        set_thread(t);
                        blockIdx.x = x, blockIdx.y = y, blockIdx.z = z;
                        thread_fn(ctx);
                    }
                }
    } else {
        L.nwaves = (L.nthreads + WAVE - 1) / WAVE;
        L.waves.reset(new Wave[L.nwaves]);
        for (unsigned w = 0; w < L.nwaves; w++)
            L.waves[w].lanes = w + 1 < L.nwaves ? WAVE : L.nthreads - w * WAVE;
        L.end_bar.reset(L.nthreads);
        prepare_block();
        while (pool.size() < L.nthreads) {
            pool.emplace_back(new Worker);
            Worker *w = pool.back().get();
            w->th = std::thread(worker_main, w, (unsigned)pool.size() - 1);
        }
        {
            std::lock_guard<std::mutex> l(done_m);
            done_left = L.nthreads;
        }
        for (unsigned t = 0; t < L.nthreads; t++) {
            {
                std::lock_guard<std::mutex> l(pool[t]->m);
                pool[t]->go = true;
            }
            pool[t]->cv.notify_one();
        }
        {
            std::unique_lock<std::mutex> l(done_m);
            done_cv.wait(l, [] { return done_left == 0; });
        }
        L.waves.reset();
        bool may = !L.synced;
        for (const char *k : ALWAYS_THREADED) may = may && L.name != k;
        if (may) {
            std::lock_guard<std::mutex> l(state_m);
            plain_loop[text] = true;
        }
    }
    free(L.lds);
    L.lds = nullptr;
}

}  // namespace hipcpu

hipError_t hipGetLastError() {
    const hipError_t e = last_error;
    last_error = hipSuccess;
    return e;
}
const char *hipGetErrorString(hipError_t e) {
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidConfiguration: return "invalid configuration argument";
    }
    return "unknown error";
}
hipError_t hipGetDeviceCount(int *n) {
    *n = 1;
    return hipSuccess;
}
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : fail(hipErrorInvalidValue); }

static hipError_t alloc_filled(void **p, size_t bytes) {
    *p = nullptr;
    if (!bytes) return hipSuccess;
    *p = malloc(bytes);
    if (!*p) return fail(hipErrorOutOfMemory);
    memset(*p, fill_byte(), bytes);
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes) { return alloc_filled(p, bytes); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return alloc_filled(p, bytes); }
hipError_t hipFree(void *p) {
    free(p);
    return hipSuccess;
}
hipError_t hipHostFree(void *p) {
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) {
    if (bytes) memmove(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind k, hipStream_t) {
    return hipMemcpy(dst, src, bytes, k);
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                            hipMemcpyKind, hipStream_t) {
    if (width > dpitch || width > spitch) return fail(hipErrorInvalidValue);
    for (size_t r = 0; r < height && width; r++)
        memmove(static_cast<char *>(dst) + r * dpitch, static_cast<const char *>(src) + r * spitch, width);
    return hipSuccess;
}
hipError_t hipMemset(void *p, int v, size_t bytes) {
    if (bytes) memset(p, v, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t) { return hipMemset(p, v, bytes); }

// streams and events are small heap objects, so that one never destroyed shows as a leak
struct ihipStream_t { int unused; };
struct ihipEvent_t { int unused; };
hipError_t hipStreamCreate(hipStream_t *s) {
    *s = new ihipStream_t{0};
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return hipStreamCreate(s); }
hipError_t hipStreamDestroy(hipStream_t s) {
    delete s;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) {
    *e = new ihipEvent_t{0};
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) {
    delete e;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) {
    *ms = 0.0f;
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void *func, hipFuncAttribute attr, int value) {
    if (attr != hipFuncAttributeMaxDynamicSharedMemorySize || value < 0 || value > 160 * 1024)
        return fail(hipErrorInvalidValue);
    std::lock_guard<std::mutex> l(state_m);
    lds_limit[func] = value;
    return hipSuccess;
}
