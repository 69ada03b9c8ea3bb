// TEST INFRASTRUCTURE: the host half of -makematrix (veryfasttree_amd/host/SeqMatrix.h) without a device - the row pool, the two
// slab buffers, the ranges and the formatter against a fake slab source whose entry (i, j) is a known function of i and j, and a
// plain single-threaded loop as the expected text.  Built and run by tests/test_makematrix_host_cpu.py, with
// -fsanitize=address,undefined when asked; needs nothing but a C++11 compiler and pthreads.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../veryfasttree_amd/host/SeqMatrix.h"

// the functions of vft_hip.h that DeviceSlabs names (never called here: the source below is the fake one)
extern "C" {
int vft_device_malloc(vft_ctx *, int64_t, void **) { abort(); }
int vft_device_free(vft_ctx *, void *) { abort(); }
int vft_host_malloc(vft_ctx *, int64_t, void **) { abort(); }
int vft_host_free(vft_ctx *, void *) { abort(); }
int vft_download_async(vft_ctx *, void *, const void *, int64_t, int32_t) { abort(); }
int vft_download_wait(vft_ctx *, int32_t) { abort(); }
int vft_seq_matrix_rows(vft_ctx *, int64_t, int64_t, int32_t, void *, int64_t, void *) { abort(); }
const char *vft_last_error(const vft_ctx *) { return ""; }
}

template <typename REAL>
static REAL entry(int64_t i, int64_t j) {
    if ((i + j) % 11 == 0) return (REAL) 0;
    if ((i * 3 + j) % 17 == 0) return (REAL) 3;
    return (REAL) ((double) ((i * 131 + j * 37) % 3001) / 1000.0 + 1e-7 * (double) (i % 5));
}

// two exactly-sized heap buffers (so that AddressSanitizer sees an overrun by one element), filled at start()
template <typename REAL>
struct FakeSlabs {
    int64_t n, ldv, rows;
    std::vector<REAL> *buf[2];
    int64_t started = 0, finished = 0;
    FakeSlabs(int64_t n, int64_t slabRows) : n(n), ldv((n + 63) & ~(int64_t) 63), rows(slabRows) {
        for (int b = 0; b < 2; b++) buf[b] = new std::vector<REAL>((size_t) (rows * ldv), (REAL) -1);
    }
    ~FakeSlabs() {
        for (int b = 0; b < 2; b++) delete buf[b];
    }
    int64_t ld() const { return ldv; }
    void start(int b, int64_t r0, int64_t r1) {
        if (r1 - r0 > rows || r0 < 0 || r1 > n || r0 >= r1) {
            fprintf(stderr, "bad slab [%lld, %lld)\n", (long long) r0, (long long) r1);
            exit(2);
        }
        for (int64_t i = r0; i < r1; i++)
            for (int64_t j = 0; j < n; j++) (*buf[b])[(size_t) ((i - r0) * ldv + j)] = entry<REAL>(i, j);
        started++;
    }
    const REAL *finish(int b) {
        finished++;
        return buf[b]->data();
    }
};

template <typename REAL>
static int check(int64_t n, int64_t slabRows) {
    std::vector<std::string> names;
    for (int64_t i = 0; i < n; i++) names.push_back("seq_" + std::to_string(i * 7));
    std::string want;
    char tmp[400];
    for (int64_t i = 0; i < n; i++) {
        want += names[(size_t) i];
        for (int64_t j = 0; j < n; j++) {
            snprintf(tmp, sizeof(tmp), " %f", (double) entry<REAL>(i, j));
            want += tmp;
        }
        want += "\n";
    }
    FILE *f = tmpfile();
    if (!f) return 3;
    const int64_t rows = slabRows > 0 ? (slabRows < n ? slabRows : n) : veryfasttree::defaultSlabRows(n, (n + 63) & ~(int64_t) 63, sizeof(REAL));
    FakeSlabs<REAL> src(n, rows);
    const veryfasttree::SeqMatrixTimes T = veryfasttree::writeSeqMatrix<REAL>(src, n, names, rows, fileno(f));
    std::string got((size_t) T.bytes, '\0');
    rewind(f);
    const size_t k = fread(&got[0], 1, got.size() + 1, f);
    fclose(f);
    const bool ok = k == want.size() && got == want && T.slabs == (n + rows - 1) / rows && src.started == T.slabs && src.finished == T.slabs;
    printf("n %lld slab %lld (%lld slabs) %s: %s\n", (long long) n, (long long) rows, (long long) T.slabs, sizeof(REAL) == 4 ? "float" : "double",
           ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    const int64_t sizes[] = {1, 2, 63, 64, 65, 130};
    const int64_t slabs[] = {0, 1, 7, 16, 17, 64, 1000};
    for (int64_t n : sizes)
        for (int64_t s : slabs) {
            bad += check<float>(n, s);
            bad += check<double>(n, s);
        }
    // repeated names are an error before anything is written
    try {
        FakeSlabs<float> src(3, 3);
        veryfasttree::writeSeqMatrix<float>(src, 3, {"a", "b", "a"}, 3, 1);
        bad++;
        printf("duplicate names: NOT refused\n");
    } catch (const std::exception &e) {
        printf("duplicate names: refused (%s)\n", e.what());
    }
    printf("failures %d\n", bad);
    return bad ? 1 : 0;
}
