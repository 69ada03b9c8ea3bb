// `-makematrix` (printDistances, NJ.tcc:274-288): the text of the all-pairs distance matrix, streamed in row slabs.
//
// The numbers come from vft_seq_matrix_rows (csrc/vft_kernels_seqmatrix.h), already narrowed, log-corrected and clamped the
// way the reference prints them; this file turns them into `name( %f){n}\n` rows and writes them to a file descriptor.
// Memory does not depend on n^2: two slabs of `slabRows` rows are in flight, each a device buffer and a page-locked host
// buffer of slabRows * ld numeric_t (ld = n rounded up to 64).  While the rows of slab k are formatted - on a pool of at
// most VFT_SM_MAX_THREADS threads, one row at a time per thread - and written, the kernel and the copy of slab k + 1 run.
// The default slab height makes those four buffers fill VFT_SM_BUDGET bytes (at least one row).
//
// The slab source is a template parameter so that the pool, the buffer arithmetic and the formatting can be run on the CPU
// against a fake source (tests/native/seqmatrix_host_check.cpp); DeviceSlabs below is the real one.
#pragma once
#include <cerrno>
#include <clocale>
#include <locale.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/vft_hip.h"

#define VFT_SM_MAX_THREADS 16
#define VFT_SM_BUDGET (256ll << 20)

namespace veryfasttree {

struct SeqMatrixTimes {
    double wait = 0, format = 0, write = 0, total = 0;   // seconds: for the device, formatting, write(2), everything
    int64_t slabs = 0, slabRows = 0, bytes = 0;
};

// Runs job(row) for row = 0 .. rows-1 on up to VFT_SM_MAX_THREADS persistent threads; run() returns when all are done.
// The size is a constant of the format, never the machine's CPU count.
class RowPool {
public:
    explicit RowPool(int nThreads) {
        if (nThreads < 1) nThreads = 1;
        if (nThreads > VFT_SM_MAX_THREADS) nThreads = VFT_SM_MAX_THREADS;
        cLocale = newlocale(LC_ALL_MASK, "C", (locale_t) 0);
        for (int t = 0; t < nThreads; t++) threads.emplace_back([this] { work(); });
    }
    ~RowPool() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        wake.notify_all();
        for (auto &t : threads) t.join();
        if (cLocale) freelocale(cLocale);
    }
    void run(int64_t rows, const std::function<void(int64_t)> &fn) {
        std::unique_lock<std::mutex> g(m);
        job = &fn;
        nRows = rows;
        next = 0;
        busy = (int) threads.size();
        generation++;
        wake.notify_all();
        done.wait(g, [this] { return busy == 0; });
        job = nullptr;
        if (!error.empty()) {
            std::string e;
            e.swap(error);
            throw std::runtime_error(e);
        }
    }
    int size() const { return (int) threads.size(); }

private:
    void work() {
        if (cLocale) uselocale(cLocale);   // "%f" with a '.', whatever the process has set
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int64_t)> *fn;
            {
                std::unique_lock<std::mutex> g(m);
                wake.wait(g, [&] { return stop || generation != seen; });
                if (stop) return;
                seen = generation;
                fn = job;
            }
            try {
                for (int64_t r = next.fetch_add(1); r < nRows; r = next.fetch_add(1)) (*fn)(r);
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> g(m);
                error = e.what();
            }
            std::lock_guard<std::mutex> g(m);
            if (--busy == 0) done.notify_all();
        }
    }
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable wake, done;
    const std::function<void(int64_t)> *job = nullptr;
    std::atomic<int64_t> next{0};
    int64_t nRows = 0;
    uint64_t generation = 0;
    int busy = 0;
    bool stop = false;
    std::string error;
    locale_t cLocale = (locale_t) 0;
};

// one row of the reference's output: the name, " %f" of every entry (NJ.tcc:284 - the kernel has made -0 and negatives 0), '\n'
template <typename REAL>
inline void formatMatrixRow(const std::string &name, const REAL *row, int64_t n, std::string &out) {
    out.clear();
    out.reserve(name.size() + (size_t) n * 10 + 2);
    out += name;
    char tmp[400];   // the longest "%f" of a double has 317 characters
    for (int64_t j = 0; j < n; j++) {
        const double v = (double) row[j];
        const int k = snprintf(tmp, sizeof(tmp), " %f", v <= 0.0 ? 0.0 : v);
        out.append(tmp, (size_t) k);
    }
    out += '\n';
}

inline void writeAll(int fd, const char *p, size_t n) {
    while (n > 0) {
        const ssize_t k = ::write(fd, p, n);
        if (k < 0) {
            if (errno == EINTR) continue;
            throw std::runtime_error(std::string("-makematrix: write failed: ") + strerror(errno));
        }
        p += k;
        n -= (size_t) k;
    }
}

inline int64_t defaultSlabRows(int64_t n, int64_t ld, size_t realSize) {
    int64_t rows = VFT_SM_BUDGET / (4 * ld * (int64_t) realSize);   // two device slabs + two host slabs
    if (rows < 1) rows = 1;
    return rows < n ? rows : n;
}

// SOURCE: ld(), start(slab buffer 0/1, r0, r1) queues the rows, finish(buffer) waits for them and returns the host rows.
template <typename REAL, typename SOURCE>
inline SeqMatrixTimes writeSeqMatrix(SOURCE &src, int64_t n, const std::vector<std::string> &names, int64_t slabRows, int fd) {
    typedef std::chrono::steady_clock clk;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    if ((int64_t) names.size() != n) throw std::runtime_error("-makematrix: one name per sequence is needed");
    {
        std::unordered_set<std::string> seen;   // the reference hashes the names first and stops at a repeat (VeryFastTreeImpl.tcc:60-61)
        for (const std::string &nm : names)
            if (!seen.insert(nm).second) throw std::runtime_error("Non-unique name '" + nm + "' in the alignment");
    }
    SeqMatrixTimes T;
    const auto t0 = clk::now();
    const int64_t ld = src.ld();
    if (slabRows <= 0) slabRows = defaultSlabRows(n, ld, sizeof(REAL));
    if (slabRows > n) slabRows = n;
    const int64_t nSlabs = (n + slabRows - 1) / slabRows;
    T.slabs = nSlabs;
    T.slabRows = slabRows;
    RowPool pool((int) (slabRows < VFT_SM_MAX_THREADS ? slabRows : VFT_SM_MAX_THREADS));
    std::vector<std::string> text((size_t) slabRows);
    auto range = [&](int64_t k, int64_t &r0, int64_t &r1) {
        r0 = k * slabRows;
        r1 = r0 + slabRows < n ? r0 + slabRows : n;
    };
    int64_t r0, r1;
    range(0, r0, r1);
    src.start(0, r0, r1);
    for (int64_t k = 0; k < nSlabs; k++) {
        if (k + 1 < nSlabs) {   // the next slab's kernel and copy run while this one is formatted
            range(k + 1, r0, r1);
            src.start((int) ((k + 1) & 1), r0, r1);
        }
        range(k, r0, r1);
        const auto a = clk::now();
        const REAL *rows = src.finish((int) (k & 1));
        const auto b = clk::now();
        const int64_t first = r0;
        pool.run(r1 - r0, [&](int64_t r) { formatMatrixRow<REAL>(names[(size_t) (first + r)], rows + r * ld, n, text[(size_t) r]); });
        const auto c = clk::now();
        for (int64_t r = 0; r < r1 - r0; r++) {
            writeAll(fd, text[(size_t) r].data(), text[(size_t) r].size());
            T.bytes += (int64_t) text[(size_t) r].size();
        }
        const auto d = clk::now();
        T.wait += secs(a, b);
        T.format += secs(b, c);
        T.write += secs(c, d);
    }
    T.total = secs(t0, clk::now());
    return T;
}

// the device as slab source: two device buffers, two page-locked host buffers, the context's stream
template <typename REAL>
class DeviceSlabs {
public:
    DeviceSlabs(vft_ctx *ctx, int64_t n, int64_t slabRows, bool logCorrect) : ctx(ctx), n(n), logCorrect(logCorrect) {
        ldv = (n + 63) & ~(int64_t) 63;
        if (slabRows <= 0) slabRows = defaultSlabRows(n, ldv, sizeof(REAL));
        if (slabRows > n) slabRows = n;
        rows = slabRows;
        const int64_t bytes = rows * ldv * (int64_t) sizeof(REAL);
        try {
            for (int b = 0; b < 2; b++) {
                chk(vft_device_malloc(ctx, bytes, &dBuf[b]));
                chk(vft_host_malloc(ctx, bytes, &hBuf[b]));
            }
        } catch (...) {
            release();
            throw;
        }
    }
    ~DeviceSlabs() { release(); }
    DeviceSlabs(const DeviceSlabs &) = delete;
    DeviceSlabs &operator=(const DeviceSlabs &) = delete;
    int64_t ld() const { return ldv; }
    int64_t slabRows() const { return rows; }
    void start(int b, int64_t r0, int64_t r1) {
        if (r1 - r0 > rows) throw std::runtime_error("-makematrix: slab larger than its buffer");
        chk(vft_seq_matrix_rows(ctx, r0, r1, logCorrect ? 1 : 0, dBuf[b], ldv, nullptr));
        chk(vft_download_async(ctx, hBuf[b], dBuf[b], (r1 - r0) * ldv * (int64_t) sizeof(REAL), b));
    }
    const REAL *finish(int b) {
        chk(vft_download_wait(ctx, b));
        return (const REAL *) hBuf[b];
    }

private:
    void chk(int rc) {
        if (rc != VFT_OK) throw std::runtime_error(vft_last_error(ctx));
    }
    void release() {
        for (int b = 0; b < 2; b++) {
            if (dBuf[b]) (void) vft_device_free(ctx, dBuf[b]);
            if (hBuf[b]) (void) vft_host_free(ctx, hBuf[b]);
            dBuf[b] = hBuf[b] = nullptr;
        }
    }
    vft_ctx *ctx;
    int64_t n, ldv = 0, rows = 0;
    bool logCorrect;
    void *dBuf[2] = {nullptr, nullptr}, *hBuf[2] = {nullptr, nullptr};
};

}   // namespace veryfasttree
