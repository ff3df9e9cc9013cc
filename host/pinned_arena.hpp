// The page-locked arena the reader pools of the `miekki` binary take their buffers from.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "miekki_hip.h"

namespace mkhost {

// Page-locked memory for the reader pools, in slabs: page-locking is a slow, serialised driver call (a pool of a few
// hundred 2 MB buffers locked one by one costs a visible part of a second at start-up), so buffers are carved out
// of 256 MB slabs and handed back to a free list; the slabs go when the arena goes.  Requests of half a slab or
// more are locked on their own.  Thread-safe (the readers allocate).
class PinnedArena {
public:
    // (a slab is page-locked AHEAD by a thread of the arena's own: sixteen readers that all stand behind one 50 ms driver call
    // whenever a slab runs out -- eleven times while 4,096 gzip'd genomes were read -- lost half a second of inflating)
    explicit PinnedArena(mk_ctx *ctx) : ctx_(ctx), filler_([this] { fill(); }) {}
    ~PinnedArena()
    {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        filler_.join();
        if (spare_) mk_host_free(ctx_, spare_);
        for (void *s : slabs_) mk_host_free(ctx_, s);
    }
    void *alloc(size_t bytes)
    {
        bytes = (bytes + 4095) / 4096 * 4096;
        if (bytes >= kSlab / 2) {
            void *p = nullptr;
            if (mk_host_alloc(ctx_, bytes, &p) != MK_OK) return nullptr;
            std::lock_guard<std::mutex> g(m_);
            big_.insert(p);
            return p;
        }
        std::unique_lock<std::mutex> g(m_);
        for (;;) {
            for (size_t i = 0; i < free_.size(); ++i)                // first fit among the blocks handed back
                if (free_[i].second >= bytes) {
                    void *p = free_[i].first;
                    sizes_[p] = free_[i].second;
                    free_.erase(free_.begin() + (long)i);
                    return p;
                }
            if (cur_ && left_ >= bytes) break;
            if (spare_) {                                            // the slab made ahead becomes the current one; the next is asked for
                slabs_.push_back(spare_);
                cur_ = (char *)spare_; left_ = kSlab;
                spare_ = nullptr; want_ = true;
                cv_.notify_all();
                break;
            }
            if (dry_) return nullptr;                                // (no more page-locked memory to be had: the caller takes ordinary memory)
            want_ = true;
            cv_.notify_all();
            const auto t0 = std::chrono::steady_clock::now();
            const uint64_t seen = released_;
            cv_.wait(g, [&] { return spare_ || dry_ || released_ != seen; });      // (or a block came back that may fit)
            lock_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        void *p = cur_;
        cur_ += bytes; left_ -= bytes;
        sizes_[p] = bytes;
        return p;
    }
    void release(void *p)
    {
        std::unique_lock<std::mutex> g(m_);
        if (big_.erase(p)) { g.unlock(); mk_host_free(ctx_, p); return; }
        auto it = sizes_.find(p);
        if (it != sizes_.end()) { free_.emplace_back(p, it->second); sizes_.erase(it); ++released_; g.unlock(); cv_.notify_all(); }
    }
    double lock_s_ = 0;                          // time callers stood waiting for a slab
    size_t n_slabs_ = 0;
private:
    static constexpr size_t kSlab = 256u << 20;
    void fill()                                   // page-locks the next slab whenever the spare one has been taken
    {
        std::unique_lock<std::mutex> g(m_);
        for (;;) {                                // (nothing until somebody asks: an arena that is hardly used locks one slab, on demand)
            cv_.wait(g, [&] { return stop_ || (want_ && !spare_ && !dry_); });
            if (stop_) return;
            want_ = false;
            g.unlock();
            void *s = nullptr;
            const bool ok = mk_host_alloc(ctx_, kSlab, &s) == MK_OK;
            g.lock();
            if (ok) { spare_ = s; ++n_slabs_; } else dry_ = true;
            cv_.notify_all();
        }
    }
    mk_ctx *ctx_;
    std::mutex m_;
    std::condition_variable cv_;
    void *spare_ = nullptr;
    bool want_ = false, dry_ = false, stop_ = false;
    uint64_t released_ = 0;
    std::vector<void *> slabs_;
    char *cur_ = nullptr;
    size_t left_ = 0;
    std::vector<std::pair<void *, size_t>> free_;
    std::unordered_map<void *, size_t> sizes_;
    std::unordered_set<void *> big_;
    std::thread filler_;                         // (last: it runs as soon as it exists)
};
inline void *pinned_alloc(void *arena, size_t bytes) { return ((PinnedArena *)arena)->alloc(bytes); }
inline void pinned_free(void *arena, void *p) { ((PinnedArena *)arena)->release(p); }

}  // namespace mkhost
