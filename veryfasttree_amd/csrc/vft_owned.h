// The owner of a context's device and pinned-host memory: every allocation is made through it, is remembered with the address of the
// member that holds it, and is released through it - one by one, back to a mark, or all at once.  No HIP in here: the four raw
// operations are defined by the program that includes this header (vft_api.hip with HIP, the CPU test with malloc / free), each
// returning 0 or that program's error code.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

int vft_raw_device_alloc(void **p, size_t bytes, bool fineGrained);   // fineGrained: the walk server's device mailbox
int vft_raw_device_free(void *p);
int vft_raw_host_alloc(void **host, void **dev, size_t bytes);        // mapped pinned memory and its device address
int vft_raw_host_free(void *host);

struct VftOwned {
    enum Kind { DEVICE, HOST };
    struct Entry {
        void *p;
        Kind kind;
        size_t bytes;             // as requested
        void **member, **alias;   // where the owner's user keeps p (and a host block's device address): nulled on release
                                  // (kept as void ** whatever the member's pointer type, and written through that: deliberate - the
                                  //  compilers this builds with let a void * store alias every object pointer, and the members are
                                  //  re-read across calls)
    };
    std::vector<Entry> live;
    int err = 0;   // the raw operation's code of the last failed allocation

    // The members must stay where they are while their allocation lives (a context's own members do; its sweep slots sit in a
    // vector that is reserved once, for as many as there can ever be).  A request of 0 bytes is one of 1 byte.
    template <typename T>
    bool device(T **member, size_t bytes, bool fineGrained = false) {
        void *p = nullptr;
        if ((err = vft_raw_device_alloc(&p, bytes ? bytes : 1, fineGrained)) != 0) return false;
        *member = (T *) p;
        live.push_back(Entry{p, DEVICE, bytes, (void **) member, nullptr});
        return true;
    }
    // ... the first `zeroed` bytes of a host block are cleared
    template <typename H, typename D>
    bool host(H **member, D **devMember, size_t bytes, size_t zeroed) {
        void *h = nullptr, *d = nullptr;
        if ((err = vft_raw_host_alloc(&h, &d, bytes ? bytes : 1)) != 0) return false;
        memset(h, 0, zeroed < bytes ? zeroed : bytes);
        *member = (H *) h;
        *devMember = (D *) d;
        live.push_back(Entry{h, HOST, bytes, (void **) member, (void **) devMember});
        return true;
    }
    // frees and forgets the allocation *member holds; false (and nothing freed) when it is null or not the owner's
    template <typename T>
    bool release(T **member) {
        for (size_t i = live.size(); i-- > 0;)
            if (*member && live[i].p == (void *) *member) {
                drop(live[i]);
                *member = nullptr;
                live.erase(live.begin() + (ptrdiff_t) i);
                return true;
            }
        return false;
    }
    // A group of allocations is made completely or not at all: take a mark, allocate, and after a failure roll back to the mark.
    // (A mark is a position: release() nothing older than it in between.)
    size_t mark() const { return live.size(); }
    void rollback(size_t mark) {
        while (live.size() > mark) {
            drop(live.back());
            live.pop_back();
        }
    }
    void release_all() { rollback(0); }   // newest first
    void count(int64_t out[2]) const {
        out[0] = (int64_t) live.size();
        out[1] = 0;
        for (const Entry &e : live) out[1] += (int64_t) e.bytes;
    }

  private:
    static void drop(const Entry &e) {
        if (e.kind == HOST) (void) vft_raw_host_free(e.p);
        else (void) vft_raw_device_free(e.p);
        *e.member = nullptr;
        if (e.alias) *e.alias = nullptr;
    }
};
