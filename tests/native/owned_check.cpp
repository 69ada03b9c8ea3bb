// The allocation owner of a context (veryfasttree_amd/csrc/vft_owned.h) over malloc / free: groups that fail at every position roll
// back to their mark, release by pointer, regrow, release-everything with the matching raw operation exactly once, and the refusal of
// a pointer the owner does not know.  Host code only; run plain and under AddressSanitizer (leaks and double frees).
#include <cstdio>
#include <cstdlib>

#include "../../veryfasttree_amd/csrc/vft_owned.h"

static long g_calls = 0, g_failAt = 0;   // the g_failAt-th allocation from now fails (0: none)
static long g_devAlloc = 0, g_devFree = 0, g_hostAlloc = 0, g_hostFree = 0, g_fine = 0;
static int failures = 0;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            failures++;                                               \
        }                                                             \
    } while (0)

// every block carries its kind in front, so that a free through the wrong raw operation is seen
static const size_t HDR = 16;
static void *tagged(size_t bytes, char kind) {
    char *p = (char *) malloc(bytes + HDR);
    if (!p) return nullptr;
    p[0] = kind;
    return p + HDR;
}
static int untag(void *p, char kind) {
    char *base = (char *) p - HDR;
    CHECK(base[0] == kind);
    free(base);
    return 0;
}
static bool fail_now() { return g_failAt && ++g_calls == g_failAt; }

int vft_raw_device_alloc(void **p, size_t bytes, bool fineGrained) {
    if (fail_now()) return 2;
    *p = tagged(bytes, 'd');
    g_devAlloc++;
    g_fine += fineGrained;
    return *p ? 0 : 2;
}
int vft_raw_device_free(void *p) {
    g_devFree++;
    return untag(p, 'd');
}
int vft_raw_host_alloc(void **host, void **dev, size_t bytes) {
    if (fail_now()) return 2;
    *host = tagged(bytes, 'h');
    if (*host) memset(*host, 0x5A, bytes);
    *dev = *host;   // (a mapped block's device address; any non-null value serves)
    g_hostAlloc++;
    return *host ? 0 : 2;
}
int vft_raw_host_free(void *host) {
    g_hostFree++;
    return untag(host, 'h');
}

// a subsystem of n buffers, every third one a host block: all of them or none
struct Sub {
    static const int MAXN = 9;
    void *dev[MAXN] = {};
    char *host[MAXN] = {}, *hostDev[MAXN] = {};
};
static bool make(VftOwned &own, Sub &s, int n) {
    const size_t mark = own.mark();
    for (int i = 0; i < n; i++) {
        const bool ok = i % 3 == 2 ? own.host(&s.host[i], &s.hostDev[i], 40 + (size_t) i, 8) : own.device(&s.dev[i], 100 + (size_t) i);
        if (!ok) {
            own.rollback(mark);
            return false;
        }
    }
    return true;
}
static bool all_null(const Sub &s) {
    for (int i = 0; i < Sub::MAXN; i++)
        if (s.dev[i] || s.host[i] || s.hostDev[i]) return false;
    return true;
}

int main() {
    int64_t cnt[2], cnt0[2];
    {
        // 1. a group that fails at every k in 1..n rolls back to the mark, and a second attempt succeeds
        VftOwned own;
        int *before = nullptr;
        CHECK(own.device(&before, 12));
        own.count(cnt0);
        CHECK(cnt0[0] == 1 && cnt0[1] == 12);
        for (int n = 1; n <= Sub::MAXN; n++)
            for (int k = 1; k <= n; k++) {
                Sub s;
                g_calls = 0;
                g_failAt = k;
                CHECK(!make(own, s, n));
                CHECK(own.err == 2);
                g_failAt = 0;
                own.count(cnt);
                CHECK(cnt[0] == cnt0[0] && cnt[1] == cnt0[1]);
                CHECK(all_null(s));
                CHECK(before != nullptr);
                CHECK(make(own, s, n));
                own.count(cnt);
                CHECK(cnt[0] == cnt0[0] + n);
                for (int i = 0; i < n; i++) CHECK(i % 3 == 2 ? (s.host[i] && s.hostDev[i] == s.host[i] && !s.dev[i]) : (s.dev[i] && !s.host[i]));
                if (n >= 3) {   // the first `zeroed` bytes of a host block are cleared, the rest is as the raw operation left it
                    CHECK(s.host[2][0] == 0 && s.host[2][7] == 0 && s.host[2][8] == 0x5A);
                }
                own.rollback((size_t) cnt0[0]);
                CHECK(all_null(s));
            }
        own.release_all();
        CHECK(before == nullptr);
        CHECK(g_devAlloc == g_devFree && g_hostAlloc == g_hostFree && g_devAlloc > 0 && g_hostAlloc > 0);
    }
    {
        // 2. release by pointer in the middle of the vector, 3. regrow keeps the count, 5. an unknown pointer is refused
        VftOwned own;
        void *a = nullptr, *b = nullptr, *c = nullptr;
        char *h = nullptr, *hd = nullptr;
        CHECK(own.device(&a, 10) && own.device(&b, 20) && own.host(&h, &hd, 30, 30) && own.device(&c, 0));
        own.count(cnt);
        CHECK(cnt[0] == 4 && cnt[1] == 60);   // (a request of 0 bytes is counted as asked)
        const long df = g_devFree, hf = g_hostFree;
        CHECK(own.release(&b));
        CHECK(b == nullptr && a && c && h && g_devFree == df + 1 && g_hostFree == hf);
        own.count(cnt);
        CHECK(cnt[0] == 3 && cnt[1] == 40);
        CHECK(!own.release(&b));   // null: nothing to release
        CHECK(own.release(&h));    // a host block, with its device address
        CHECK(h == nullptr && hd == nullptr && g_hostFree == hf + 1 && g_devFree == df + 1);
        for (size_t want = 64; want <= 4096; want *= 4) {   // regrow: release, then allocate larger
            CHECK(own.release(&a));
            CHECK(own.device(&a, want));
            own.count(cnt);
            CHECK(cnt[0] == 2 && cnt[1] == (int64_t) want);
        }
        int local = 0;
        void *stranger = &local, *inner = (char *) a + 8;
        const long df2 = g_devFree, hf2 = g_hostFree;
        CHECK(!own.release(&stranger) && stranger == &local);
        CHECK(!own.release(&inner) && inner == (char *) a + 8);
        CHECK(g_devFree == df2 && g_hostFree == hf2);
        own.count(cnt);
        CHECK(cnt[0] == 2);
        own.release_all();
        CHECK(a == nullptr && c == nullptr);
    }
    {
        // 4. release-everything after a mix of kinds: each block through its own raw operation (untag checks the kind), exactly once,
        //    newest first
        VftOwned own;
        const long da = g_devAlloc, df = g_devFree, ha = g_hostAlloc, hf = g_hostFree, fine = g_fine;
        void *d[6] = {};
        char *h[5] = {}, *hd[5] = {};
        for (int i = 0; i < 5; i++) {
            CHECK(own.device(&d[i], 7 + (size_t) i));
            CHECK(own.host(&h[i], &hd[i], 9 + (size_t) i, 0));
        }
        CHECK(own.device(&d[5], 64, true));   // fine-grained device memory is released as device memory
        CHECK(g_fine == fine + 1);
        CHECK(own.live.front().p == d[0] && own.live.back().p == d[5]);
        own.release_all();
        CHECK(g_devAlloc - da == 6 && g_devFree - df == 6 && g_hostAlloc - ha == 5 && g_hostFree - hf == 5);
        own.count(cnt);
        CHECK(cnt[0] == 0 && cnt[1] == 0);
        for (int i = 0; i < 6; i++) CHECK(d[i] == nullptr);
        for (int i = 0; i < 5; i++) CHECK(h[i] == nullptr && hd[i] == nullptr);
        own.release_all();   // nothing left: nothing freed twice
        CHECK(g_devFree - df == 6 && g_hostFree - hf == 5);
    }
    printf("device %ld / %ld host %ld / %ld (allocated / freed)\n", g_devAlloc, g_devFree, g_hostAlloc, g_hostFree);
    CHECK(g_devAlloc == g_devFree && g_hostAlloc == g_hostFree);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
