// arena_check.cpp - csrc/arena.h against a brute-force model (tests/test_arena.py builds this with -fsanitize=address,undefined and runs it).
// The model is a plain list of live blocks; "first fit" is restated as: the lowest 256-aligned offset at which the block overlaps no live
// block and ends inside the arena.  Every step compares the arena with the model and checks the arena's own lists.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <random>
#include <vector>
#include "arena.h"

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

struct Live { long long off, size; void* p; };

static long long model_fit(const std::vector<Live>& live, long long size, long long cap) {
    std::vector<long long> cand{0};
    for (const Live& b : live) cand.push_back(b.off + b.size);
    long long best = -1;
    for (long long o : cand) {
        if (o + size > cap) continue;
        bool free_here = true;
        for (const Live& b : live) free_here = free_here && (o + size <= b.off || b.off + b.size <= o);
        if (free_here && (best < 0 || o < best)) best = o;
    }
    return best;
}

static void check_lists(const Arena& a, const std::vector<Live>& live, long long cap, long long peak) {
    CHECK(a.peak == peak, "peak %lld, model %lld", a.peak, peak);
    CHECK(a.live.size() == live.size(), "%zu live blocks, model %zu", a.live.size(), live.size());
    for (const Live& b : live) {
        bool found = false;
        for (const Arena::Blk& x : a.live) found = found || (x.off == b.off && x.size == b.size);
        CHECK(found, "live block %lld + %lld is not in the arena's list", b.off, b.size);
    }
    // the free list: sorted, coalesced, and together with the live blocks an exact cover of [0, cap)
    long long total = 0;
    for (size_t i = 0; i < a.free_list.size(); ++i) {
        const Arena::Blk& f = a.free_list[i];
        CHECK(f.size > 0 && f.off % 256 == 0 && f.size % 256 == 0, "free block %lld + %lld", f.off, f.size);
        if (i) CHECK(a.free_list[i - 1].off + a.free_list[i - 1].size < f.off, "free blocks %zu and %zu touch or are out of order", i - 1, i);
        for (const Live& b : live) CHECK(f.off + f.size <= b.off || b.off + b.size <= f.off, "free block %lld overlaps live block %lld", f.off, b.off);
        total += f.size;
    }
    for (size_t i = 0; i < live.size(); ++i) {
        for (size_t j = 0; j < i; ++j)
            CHECK(live[i].off + live[i].size <= live[j].off || live[j].off + live[j].size <= live[i].off, "live blocks %lld and %lld overlap", live[i].off, live[j].off);
        total += live[i].size;
    }
    CHECK(total == cap, "free + live bytes %lld, capacity %lld", total, cap);
}

// Drives one arena through `steps` seeded operations; returns the offset of every allocation (-1: refused).
static std::vector<long long> drive(void* base, long long cap, bool dry, unsigned seed, int steps, long long max_request) {
    Arena a;
    a.reset(base, dry ? 0 : cap, dry);
    const long long model_cap = dry ? (1LL << 60) : cap;
    char* const origin = dry ? (char*)0x100000 : (char*)base;
    std::mt19937 rng(seed);
    auto pick = [&](long long n) { return (long long)(rng() % (unsigned long long)n); };
    std::vector<Live> live;
    std::vector<void*> stale;                    // pointers released earlier: releasing them again must change nothing
    std::vector<long long> offsets;
    long long peak = 0;
    int refused = 0;
    for (int s = 0; s < steps; ++s) {
        const int op = (int)pick(100);
        if (op < (live.size() < 48 ? 55 : 40) || live.empty()) {      // (some fifty blocks live at a time, as in a forward)
            static const long long edge[] = {0, 1, 255, 256, 257, 511, 512, 4096};
            long long bytes = op < 10 ? edge[pick(8)] : (op < 50 ? 1 + pick(65536) : 1 + pick(max_request));
            const long long size = bytes == 0 ? 256 : (bytes + 255) / 256 * 256;
            const long long want = model_fit(live, size, model_cap);
            void* p = a.alloc(bytes);
            CHECK((p == nullptr) == (want < 0), "alloc(%lld): arena %s, model offset %lld", bytes, p ? "placed it" : "refused", want);
            CHECK(!(dry && !p), "a dry arena refused %lld bytes", bytes);
            offsets.push_back(p ? (char*)p - origin : -1);
            if (!p) { ++refused; check_lists(a, live, model_cap, peak); continue; }
            CHECK((char*)p - origin == want, "alloc(%lld) at %lld, first fit is %lld", bytes, (long long)((char*)p - origin), want);
            CHECK(want % 256 == 0 && ((uintptr_t)p & 255) == ((uintptr_t)origin & 255), "offset %lld is not 256-aligned", want);
            CHECK(a.live.back().off == want && a.live.back().size == size, "alloc(%lld) took %lld bytes, expected %lld", bytes, a.live.back().size, size);
            live.push_back({want, size, p});
            peak = std::max(peak, want + size);
        } else if (op < 90) {
            const size_t i = (size_t)pick((long long)live.size());
            a.release(live[i].p);
            stale.push_back(live[i].p);
            live.erase(live.begin() + i);
        } else if (op < 93) {
            a.release(nullptr);
        } else if (op < 97 && !live.empty()) {
            a.release((char*)live[(size_t)pick((long long)live.size())].p + 128);      // inside a live block, not its start
        } else if (!stale.empty()) {
            void* p = stale[(size_t)pick((long long)stale.size())];
            bool is_live = false;
            for (const Live& b : live) is_live = is_live || b.p == p;
            if (!is_live) a.release(p);                                                  // a second release of a block that is gone
        }
        check_lists(a, live, model_cap, peak);
    }
    if (!dry) CHECK(refused > 0 || max_request < cap / 64, "the tight arena never refused a request: the sequence does not reach the limit");
    while (!live.empty()) {
        const size_t i = (size_t)pick((long long)live.size());
        a.release(live[i].p);
        live.erase(live.begin() + i);
        check_lists(a, live, model_cap, peak);
    }
    CHECK(a.free_list.size() == 1 && a.free_list[0].off == 0 && a.free_list[0].size == model_cap, "releasing everything left %zu free blocks", a.free_list.size());
    std::printf("cap %lld dry %d seed %u: %d steps, %zu allocations, %d refused, peak %lld\n", cap, (int)dry, seed, steps, offsets.size(), refused, peak);
    return offsets;
}

int main() {
    const int steps = 4000;
    const long long tight = 1 << 20, ample = 256LL << 20;
    void* small = std::malloc((size_t)tight);
    void* big = std::malloc((size_t)ample);          // never touched: the arena hands out addresses, nobody writes through them here
    CHECK(small && big, "malloc");
    for (unsigned seed = 1; seed <= 3; ++seed) {
        drive(small, tight, false, seed, steps, tight / 2);                  // requests up to half the arena: refusals happen
        const std::vector<long long> real = drive(big, ample, false, seed + 100, steps, 262144);
        const std::vector<long long> dry = drive(nullptr, 0, true, seed + 100, steps, 262144);
        CHECK(real == dry, "a dry arena and an ample real one placed the same requests differently");
        for (long long o : real) CHECK(o >= 0, "the ample arena refused a request");
    }
    // a zero-byte request gets a block of 256 bytes; an exact fit leaves no free block; one byte more is refused
    Arena a;
    a.reset(small, 1024, false);
    void* z = a.alloc(0);
    CHECK(z == small && a.live.back().size == 256 && a.peak == 256, "alloc(0)");
    CHECK(a.alloc(769) == nullptr && a.peak == 256, "769 bytes fit into 768");
    void* rest = a.alloc(768);
    CHECK(rest == (char*)small + 256 && a.free_list.empty() && a.peak == 1024, "exact fit");
    CHECK(a.alloc(0) == nullptr, "a full arena placed a block");
    a.release(z); a.release(rest);
    CHECK(a.free_list.size() == 1 && a.free_list[0].size == 1024 && a.live.empty(), "coalescing");
    std::free(small); std::free(big);
    std::printf("arena: ok\n");
    return 0;
}
