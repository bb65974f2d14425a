// arena.h - the activation allocator of the UNet executor (runtime.hip): first fit over a free list sorted by offset, 256-byte blocks,
// neighbours coalesced on release.  It decides the address of every activation of a forward; `dry` counts bytes without memory behind
// them (icd_unet_workspace_bytes).  Plain C++, no HIP: tests/test_arena.py drives it against a brute-force model under sanitizers.
#pragma once
#include <algorithm>
#include <vector>

struct __attribute__((visibility("hidden"))) Arena {      // (internal to the library: not an exported symbol)
    char* base = nullptr;
    long long cap = 0, peak = 0;
    bool dry = false;
    struct Blk { long long off, size; };
    std::vector<Blk> free_list;   // sorted by offset
    std::vector<Blk> live;
    void reset(void* b, long long c, bool d) {
        base = (char*)b; cap = c; dry = d; peak = 0;
        free_list.clear(); live.clear();
        free_list.push_back({0, d ? (1LL << 60) : c});
    }
    void* alloc(long long bytes) {
        bytes = (bytes + 255) & ~255LL;
        if (bytes == 0) bytes = 256;
        for (size_t i = 0; i < free_list.size(); ++i) {
            if (free_list[i].size >= bytes) {
                const long long off = free_list[i].off;
                free_list[i].off += bytes; free_list[i].size -= bytes;
                if (free_list[i].size == 0) free_list.erase(free_list.begin() + i);
                live.push_back({off, bytes});
                peak = std::max(peak, off + bytes);
                return (dry ? (char*)0x100000 : base) + off;
            }
        }
        return nullptr;
    }
    void release(void* p) {
        if (!p) return;
        const long long off = (char*)p - (dry ? (char*)0x100000 : base);
        for (size_t i = 0; i < live.size(); ++i)
            if (live[i].off == off) {
                Blk b = live[i];
                live.erase(live.begin() + i);
                auto it = std::lower_bound(free_list.begin(), free_list.end(), b,
                                           [](const Blk& x, const Blk& y) { return x.off < y.off; });
                it = free_list.insert(it, b);
                if (it + 1 != free_list.end() && it->off + it->size == (it + 1)->off) {
                    it->size += (it + 1)->size; free_list.erase(it + 1);
                }
                if (it != free_list.begin() && (it - 1)->off + (it - 1)->size == it->off) {
                    (it - 1)->size += it->size; free_list.erase(it);
                }
                return;
            }
    }
};
