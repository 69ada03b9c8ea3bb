// How a call's arguments are laid out in one byte buffer, whether that buffer is a slice of the host-mapped ring or the device scratch,
// and which nodes of an id list are stale.  Arithmetic and host vectors only, no HIP in here: vft_api.hip moves the bytes (its Stage),
// tests/native/staging_check.cpp checks this header as a stand-alone program.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#define VFT_SMALL_BYTES ((size_t) 256u << 10)   // what goes through the host-mapped ring unless a site says otherwise

inline size_t vft_pad256(size_t bytes) { return (bytes + 255) & ~(size_t) 255; }   // the granule of the ring and of most regions

// Regions of one buffer, added in order: add() returns the region's offset, total() the end of the last region.
struct VftLayout {
    size_t end = 0;
    size_t add(size_t bytes, size_t align = 1) {
        const size_t at = (end + align - 1) / align * align;
        end = at + bytes;
        return at;
    }
    size_t total() const { return end; }
};
// the one rule of the two transport paths: a buffer of `total` bytes is a slice of the ring up to the site's limit, the scratch beyond
// (the ring hands out multiples of 256 bytes and every limit is one, so a total that ends short of its padding decides the same)
inline bool vft_takes_ring(size_t total, size_t limit) { return total <= limit; }

// setCriterion's lazy refresh (NJ.tcc:1092-1098) is applied to the DISTINCT stale nodes a call names, found on the host-mapped
// mirror of the nodes' stamps (it can only lag towards "staler").  One set per call: constructing it starts a new epoch of the
// marks (no id is marked; a wrapped epoch clears them), add() appends each id that is stale and not yet marked to `out`.
struct VftStaleSet {
    const int32_t *nOut;           // the stamp mirror
    std::vector<uint32_t> &mark;   // == epoch: already in `out`
    int32_t *pos;                  // (optional) pos[v]: where v stands in `out`, valid while has(v)
    uint32_t epoch;
    int64_t nActive, nDiffAllow;
    std::vector<int64_t> &out;

    VftStaleSet(const int32_t *nOut_, std::vector<uint32_t> &mark_, uint32_t &epoch_, size_t nNodes, int64_t nActive_, int64_t nDiffAllow_,
                std::vector<int64_t> &out_, std::vector<int32_t> *pos_ = nullptr)
        : nOut(nOut_), mark(mark_), pos(nullptr), nActive(nActive_), nDiffAllow(nDiffAllow_), out(out_) {
        out.clear();
        if (mark.size() != nNodes) mark.assign(nNodes, 0u);
        if (++epoch_ == 0u) {
            std::fill(mark.begin(), mark.end(), 0u);
            epoch_ = 1u;
        }
        epoch = epoch_;
        if (pos_) {
            if (pos_->size() != nNodes) pos_->assign(nNodes, -1);
            pos = pos_->data();
        }
    }
    // lazy: the stamp is more than nDiffAllow above nActive; forced (setOutDistance, NJ.tcc:1012-1015): the stamp is not nActive
    // (the stamp first: nearly every id is fresh, and its mark - a second cache miss per id of a long list - is then never looked at)
    void add(int64_t v, bool forced = false) {
        if (v < 0) return;
        if (forced ? (int64_t) nOut[v] == nActive : !((int64_t) nOut[v] - nActive > nDiffAllow)) return;
        if (mark[(size_t) v] == epoch) return;
        mark[(size_t) v] = epoch;
        if (pos) pos[v] = (int32_t) out.size();
        out.push_back(v);
    }
    void add(const int64_t *ids, int64_t n, bool forced = false) {
        for (int64_t t = 0; t < n; t++) add(ids[t], forced);
    }
    bool has(int64_t v) const { return mark[(size_t) v] == epoch; }
    int32_t where(int64_t v) const { return has(v) ? pos[v] : -1; }
};
