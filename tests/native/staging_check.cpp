// The argument layouts and the stale-node collector of the C ABI (veryfasttree_amd/csrc/vft_staging.h) as a stand-alone program:
// regions never overlap and honour their alignment, every dual-path entry point takes the ring up to exactly the list length it
// always has (the conditions of the hand-carved layouts are restated here as plain arithmetic), and the collector reports every
// distinct stale id once, in first-seen order, across an epoch wrap.  Host code only; run plain and under AddressSanitizer.
#include <cstdio>
#include <cstdlib>

#include "../../veryfasttree_amd/csrc/vft_staging.h"

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            failures++;                                               \
        }                                                             \
    } while (0)

static size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

// ------------------------------------------------------------------------------------------------ the layout
static void check_layout() {
    struct Region {
        size_t bytes, align;
    };
    const Region regions[] = {{24, 1}, {0, 256}, {7, 8}, {1, 1}, {300, 256}, {0, 1}, {5, 64}, {8, 8}, {0, 256}, {0, 256}, {13, 16}};
    VftLayout L;
    CHECK(L.total() == 0);
    size_t prevEnd = 0;
    for (const Region &r : regions) {
        const size_t before = L.total(), at = L.add(r.bytes, r.align);
        CHECK(at % r.align == 0);                 // honours its alignment
        CHECK(at >= prevEnd);                     // never overlaps what came before
        CHECK(at - before < r.align);             // no more padding than the alignment needs
        CHECK(L.total() == at + r.bytes);         // total() is the end of the last region
        if (r.bytes == 0) CHECK(L.total() == at); // a zero-byte region takes no space beyond alignment
        prevEnd = at + r.bytes;
    }
    VftLayout M;   // aligned zero-byte regions in a row: the second one is free
    M.add(3);
    const size_t a = M.add(0, 256), b = M.add(0, 256);
    CHECK(a == 256 && b == 256 && M.total() == 256);
    CHECK(vft_pad256(0) == 0 && vft_pad256(1) == 256 && vft_pad256(256) == 256 && vft_pad256(257) == 512);
    CHECK(vft_takes_ring(VFT_SMALL_BYTES, VFT_SMALL_BYTES) && !vft_takes_ring(VFT_SMALL_BYTES + 1, VFT_SMALL_BYTES));
}

// ------------------------------------------------------------------------------------------------ ring or scratch, site by site
// each recipe is the one of the entry point in vft_api.hip; `limit` its ring limit
static size_t total_pair_loglk(size_t n) {
    VftLayout L;
    for (int k = 0; k < 4; k++) L.add(n * 8);   // a | b | length | loglk (no per-site likelihoods)
    return L.total();
}
static size_t total_posterior_profiles(size_t n) {
    VftLayout L;
    for (int k = 0; k < 5; k++) L.add(n * 8);   // out | a | b | len1 | len2
    return L.total();
}
static size_t total_posterior_profiles_blen(size_t n) {
    VftLayout L;
    for (int k = 0; k < 7; k++) L.add(n * 8);   // out | a | b | lenIdxA | lenIdxB | l1 | l2
    return L.total();
}
static size_t total_average_profiles(size_t n) {
    VftLayout L;
    for (int k = 0; k < 4; k++) L.add(n * 8, 256);   // out | a | b | bionj
    L.add(0, 256);
    return L.total();
}
static size_t total_pair_distances(size_t n, size_t rs, size_t nStale) {
    VftLayout L;
    L.add(n * 8, 256);   // i
    L.add(n * 8, 256);   // j
    for (int k = 0; k < 3; k++) L.add(n * rs, 256);   // dist | weight | crit
    L.add(nStale * 8, 256);
    L.add(n * 8, 256);   // wait indices
    L.add(0, 256);
    return L.total();
}
static size_t total_nodes_set(size_t n, size_t rs) {
    VftLayout L;
    L.add(n * 8, 256);
    L.add(n * 4, 256);
    L.add(n * rs, 256);
    return L.add(0, 256);
}

template <typename Total, typename Parent>
static void check_boundary(const char *site, size_t expect, size_t limit, Total total, Parent parentTakesRing) {
    size_t last = 0;
    for (size_t n = 1; n <= 40000; n++) {
        const bool ring = vft_takes_ring(total(n), limit);
        if (ring != parentTakesRing(n)) {
            printf("FAILED %s: n = %zu takes the %s\n", site, n, ring ? "ring" : "scratch");
            failures++;
            return;
        }
        if (ring) {
            CHECK(last == n - 1);   // (one boundary: the ring below it, the scratch above)
            last = n;
        }
    }
    if (expect) CHECK(last == expect);
    CHECK(vft_takes_ring(total(last), limit) && !vft_takes_ring(total(last + 1), limit));
    printf("%-44s largest list on the ring: %zu\n", site, last);
}

static void check_sites() {
    const size_t S = VFT_SMALL_BYTES;
    CHECK(S == (size_t) 256 << 10);
    check_boundary("vft_pair_loglk", 16384, 2 * S, total_pair_loglk, [&](size_t n) { return 4 * 8 * n <= 2 * S; });
    check_boundary("vft_posterior_profiles", 13107, 2 * S, total_posterior_profiles, [&](size_t n) { return 5 * 8 * n <= 2 * S; });
    check_boundary("vft_posterior_profiles_blen", 4681, S, total_posterior_profiles_blen, [&](size_t n) { return 7 * 8 * n <= S; });
    check_boundary("vft_average_profiles", 8192, S, total_average_profiles, [&](size_t n) { return 4 * pad256(8 * n) <= S; });
    for (size_t rs = 4; rs <= 8; rs += 4)
        for (int fullyStale = 0; fullyStale < 2; fullyStale++) {
            char name[64];
            snprintf(name, sizeof(name), "pair_distances f%zu, nStale = %s", rs * 8, fullyStale ? "2n" : "0");
            auto nStale = [=](size_t n) { return fullyStale ? 2 * n : (size_t) 0; };
            check_boundary(
                name, 0, S, [&](size_t n) { return total_pair_distances(n, rs, nStale(n)); },
                [&](size_t n) { return 2 * pad256(8 * n) + 3 * pad256(rs * n) + pad256(8 * nStale(n)) + pad256(8 * n) <= S; });
            // ... and every offset is the hand-carved one
            for (size_t n : {(size_t) 1, (size_t) 33, (size_t) 2047, (size_t) 5000})
                CHECK(total_pair_distances(n, rs, nStale(n)) == 2 * pad256(8 * n) + 3 * pad256(rs * n) + pad256(8 * nStale(n)) + pad256(8 * n));
        }
    for (size_t rs = 4; rs <= 8; rs += 4)
        check_boundary(rs == 4 ? "vft_nj_engine_nodes_set f32" : "vft_nj_engine_nodes_set f64", 0, S, [&](size_t n) { return total_nodes_set(n, rs); },
                       [&](size_t n) { return pad256(8 * n) + pad256(4 * n) + pad256(rs * n) <= S; });
}

// ------------------------------------------------------------------------------------------------ the collector
static void check_collector() {
    const size_t N = 64;
    const int64_t nActive = 100, nDiffAllow = 10;
    std::vector<int32_t> nOut(N, (int32_t) nActive);   // fresh
    std::vector<uint32_t> mark;
    std::vector<int32_t> pos;
    std::vector<int64_t> out{7, 7, 7};   // (a set starts empty whatever the vector held)
    uint32_t epoch = 0;
    {   // nothing stale: nothing reported, by either rule
        VftStaleSet set(nOut.data(), mark, epoch, N, nActive, nDiffAllow, out);
        const int64_t ids[] = {3, 9, 3, -1, 63};
        set.add(ids, 5);
        set.add(ids, 5, true);
        CHECK(out.empty() && epoch == 1 && mark.size() == N);
    }
    nOut[5] = 111;    // lazy-stale (111 - 100 > 10) and forced-stale
    nOut[9] = 110;    // within the allowance: forced-stale only
    nOut[20] = 101;   // forced-stale only
    nOut[40] = 500;
    nOut[41] = 99;    // below nActive: forced-stale only
    {   // duplicates once, first-seen order, negatives skipped, positions recorded
        VftStaleSet set(nOut.data(), mark, epoch, N, nActive, nDiffAllow, out, &pos);
        const int64_t ids[] = {40, -1, 5, 9, 40, 20, 5, 41, -7, 0};
        set.add(ids, 10);
        CHECK(out.size() == 2 && out[0] == 40 && out[1] == 5);
        CHECK(set.has(40) && set.has(5) && !set.has(9) && !set.has(0));
        CHECK(set.where(40) == 0 && set.where(5) == 1 && set.where(9) == -1);
        for (size_t k = 0; k < out.size(); k++) CHECK(pos[(size_t) out[k]] == (int32_t) k);   // positions index the output
        set.add(ids, 10);   // a second pass over the same list adds nothing
        CHECK(out.size() == 2);
    }
    {   // the forced rule differs from the lazy one exactly where the stamp is off nActive by no more than the allowance (or below it)
        for (int32_t stamp = 95; stamp <= 115; stamp++) {
            nOut[30] = stamp;
            std::vector<int64_t> lazy, forced;
            VftStaleSet a(nOut.data(), mark, epoch, N, nActive, nDiffAllow, lazy);
            a.add(30);
            VftStaleSet b(nOut.data(), mark, epoch, N, nActive, nDiffAllow, forced);
            b.add(30, true);
            const int64_t diff = (int64_t) stamp - nActive;
            CHECK(lazy.size() == (size_t) (diff > nDiffAllow));
            CHECK(forced.size() == (size_t) (diff != 0));
            if (diff > 0) CHECK((lazy.size() != forced.size()) == (diff <= nDiffAllow));
        }
        nOut[30] = (int32_t) nActive;
    }
    {   // forced entries first, then the lazy rest: one list, an id forced and named again is there once
        VftStaleSet set(nOut.data(), mark, epoch, N, nActive, nDiffAllow, out, &pos);
        const int64_t force[] = {9, 5, 9}, ids[] = {5, 40, 9, 20};
        set.add(force, 3, true);
        const size_t nForced = out.size();
        set.add(ids, 4);
        CHECK(nForced == 2 && out.size() == 3 && out[0] == 9 && out[1] == 5 && out[2] == 40);
        CHECK(set.where(9) == 0 && set.where(5) == 1 && set.where(40) == 2 && set.where(20) == -1);
    }
    {   // the epoch wraps: the marks of 2^32 - 1 earlier sets are cleared, and the sets behind the wrap report every stale id once
        epoch = 0xFFFFFFFEu;
        {
            VftStaleSet last(nOut.data(), mark, epoch, N, nActive, nDiffAllow, out);
            last.add(40);
            last.add(5);
            CHECK(epoch == 0xFFFFFFFFu && out.size() == 2 && mark[40] == 0xFFFFFFFFu);
        }
        mark[6] = 1u;   // a mark as old as the epoch numbers that come round again
        nOut[6] = 400;
        const int64_t ids[] = {5, 6, 40, 5, 6};
        for (int call = 0; call < 2; call++) {
            VftStaleSet set(nOut.data(), mark, epoch, N, nActive, nDiffAllow, out);
            CHECK(epoch == (uint32_t) (1 + call));
            set.add(ids, 5);
            CHECK(out.size() == 3 && out[0] == 5 && out[1] == 6 && out[2] == 40);
        }
    }
    {   // a context with another node count: the marks are sized anew
        VftStaleSet set(nOut.data(), mark, epoch, N / 2, nActive, nDiffAllow, out, &pos);
        CHECK(mark.size() == N / 2 && pos.size() == N / 2);
        set.add(5);
        CHECK(out.size() == 1);
    }
}

int main() {
    check_layout();
    check_sites();
    check_collector();
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
