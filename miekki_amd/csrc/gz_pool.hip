// GzPool (gz_pool.hpp): what a context keeps for the inflater between batches.
#include <algorithm>
#include <thread>

#include "mk_internal.hpp"

namespace mk {

GzCounts g_gz_counts;

// pools that keep blocks (for gz_release_idle_blocks).  A pool enters with the first block it is given and leaves -- in trim --
// only when none of its block makers is at work any more: nothing can put it back behind its owner's back.
// (Order of locks: the registry's before a pool's, never the other way round.)
static std::mutex g_pools_m;
static std::vector<GzPool *> g_pools;

// (a reader thread selects the device when it is not the thread's current one, not with every call: sixteen readers at five
// runtime calls a file stood in line for the runtime's lock)
bool GzPool::use_device() const
{
    int current = -1;                                               // (asked, not remembered: other calls of this thread may have chosen another)
    if (hipGetDevice(&current) == hipSuccess && current == device) return true;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return false; }
    return true;
}

GzPool::Block *GzPool::fit(Role role, uint64_t need)               // (m_ is held) the smallest kept block of the role with room for `need`
{
    Block *best = nullptr;
    for (Block &b : kept_) if (b.role == role && b.blk.cap >= need && (!best || b.blk.cap < best->blk.cap)) best = &b;
    return best;
}

DevArray<uint8_t> GzPool::take(Role role, uint64_t need)
{
    std::unique_lock<std::mutex> g(m_);
    Block *best = fit(role, need);
    if (!best) { g.unlock(); return make(need); }
    DevArray<uint8_t> blk = std::move(best->blk);
    kept_.erase(kept_.begin() + (best - kept_.data()));
    return blk;
}

// (not DevArray::alloc: when memory is short THIS pool's kept blocks make room and the allocation is tried once more)
DevArray<uint8_t> GzPool::make(uint64_t need)
{
    DevArray<uint8_t> blk;
    const uint64_t want = need + need / 8 + 4096;
    GzCounts::Timed count{g_gz_counts.malloc_us, &g_gz_counts.malloc_n};
    if (hipMalloc((void **)&blk.p, want) != hipSuccess) {
        (void)hipGetLastError();
        { std::lock_guard<std::mutex> g(m_); kept_.clear(); }
        if (hipMalloc((void **)&blk.p, want) != hipSuccess) { (void)hipGetLastError(); blk.p = nullptr; return blk; }
    }
    blk.cap = want;
    return blk;
}

void GzPool::give(Role role, DevArray<uint8_t> &&blk)
{
    if (!blk.p) return;
    { std::lock_guard<std::mutex> g(g_pools_m); if (!registered_) g_pools.push_back(this); registered_ = true; }
    std::lock_guard<std::mutex> g(m_);
    kept_.push_back(Block{std::move(blk), role});
}

// (an allocation of gigabytes now and then takes a second -- the driver's doing, seen in one run of two: the blocks of the NEXT
// batch are made on a thread of their own while this one is being filled, so that only a context's first batch can stand
// waiting for one)
void GzPool::make_ahead(uint64_t need_input, uint64_t need_text)
{
    { std::lock_guard<std::mutex> g(m_); if (closing_) return; ++making_; }
    std::thread([this, need_input, need_text] {
        if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
        else for (Role role : {Role::InputTokens, Role::Text}) {
            const uint64_t need = role == Role::InputTokens ? need_input : need_text;
            { std::lock_guard<std::mutex> g(m_); if (closing_ || fit(role, need)) continue; }
            give(role, make(need));
        }
        std::lock_guard<std::mutex> g(m_);
        --making_;
        cv_.notify_all();
    }).detach();
}

void GzPool::quiesce() { std::unique_lock<std::mutex> g(m_); cv_.wait(g, [&] { return making_ == 0; }); }

// every pool's idle blocks back to the device; returns the bytes given back
uint64_t gz_release_idle_blocks()
{
    uint64_t freed = 0;
    int dev = 0;
    const bool have_dev = hipGetDevice(&dev) == hipSuccess;
    std::lock_guard<std::mutex> gk(g_pools_m);
    for (GzPool *p : g_pools) {
        std::lock_guard<std::mutex> g(p->m_);
        if (p->kept_.empty()) continue;
        (void)hipSetDevice(p->device);
        for (const GzPool::Block &b : p->kept_) freed += b.blk.cap;
        p->kept_.clear();
    }
    if (have_dev) (void)hipSetDevice(dev);
    return freed;
}

// Page-locked staging for a run's small copies (stream tables, block starts, segments): a copy to or from ordinary memory
// is a synchronous call inside the runtime -- it waits for everything queued on its stream -- and several batches unpacked
// by threads of their own then take turns instead of running side by side (measured: six batches of 128 files in flight
// finished no faster than one after the other).
PinnedArray<uint8_t> GzPool::pin_take(uint64_t need)
{
    uint64_t want = 1ull << 20;
    while (want < need) want <<= 1;
    PinnedArray<uint8_t> pin;
    {
        std::lock_guard<std::mutex> g(m_);
        for (PinnedArray<uint8_t> &kept : pins_)
            if (kept.cap == want) { pin = std::move(kept); pins_.erase(pins_.begin() + (&kept - pins_.data())); return pin; }
    }
    if (pin.alloc(want) != MK_OK) (void)hipGetLastError();
    return pin;
}

void GzPool::pin_give(PinnedArray<uint8_t> &&pin) { std::lock_guard<std::mutex> g(m_); if (pin.p) pins_.push_back(std::move(pin)); }

void *GzPool::lend()
{
    (void)use_device();
    Piece got;
    bool wait = false;
    {
        std::lock_guard<std::mutex> g(m_);
        if (!free_.empty()) { got = std::move(free_.back()); free_.pop_back(); }
        else if (made_ < kStagePieces) ++made_;
        else if (!busy_.empty()) { got = std::move(busy_.front()); busy_.pop_front(); wait = true; }
        else return nullptr;                                          // (every piece is in some caller's hands)
    }
    if (!got.mem) {
        got.mem.reset(pinned_alloc(kStagePiece));
        if (!got.mem || got.ev.create(hipEventBlockingSync | hipEventDisableTiming) != MK_OK) {
            (void)hipGetLastError();
            std::lock_guard<std::mutex> g(m_);
            --made_;
            return nullptr;
        }
    } else if (wait) {
        GzCounts::Timed count{g_gz_counts.stage_wait_us, &g_gz_counts.stage_waits};
        // the oldest queued copy: done soonest -- usually long done (a blocking wait costs a sleep even then: ask first)
        if (hipEventQuery(got.ev) != hipSuccess) { (void)hipGetLastError(); (void)hipEventSynchronize(got.ev); }
    }
    std::lock_guard<std::mutex> g(m_);
    held_.push_back(std::move(got));
    return held_.back().mem.get();
}

bool GzPool::claim(const void *data, Piece &piece, hipStream_t &up_k, uint32_t &k_up)
{
    std::lock_guard<std::mutex> g(m_);
    for (Piece &h : held_)
        if (h.mem.get() == data) { piece = std::move(h); held_.erase(held_.begin() + (&h - held_.data())); break; }
    if (!piece.mem) return false;
    k_up = up_next_++ % 4u;
    if (!up[k_up] && (!use_device() || up[k_up].create(hipStreamNonBlocking) != MK_OK)) (void)hipGetLastError();
    up_k = up[k_up];                                                  // (null: none could be made, and the put fails)
    return true;
}

void GzPool::take_back(Piece &&piece, bool queued)                  // (no piece: nothing to do)
{
    std::lock_guard<std::mutex> g(m_);
    if (piece.mem) { if (queued) busy_.push_back(std::move(piece)); else free_.push_back(std::move(piece)); }
}

// (after a build, before the queries' buffers are sized; when the context goes)  Block makers at work finish first and no new
// one starts meanwhile; only then does the pool leave the registry, and everything kept goes.
void GzPool::trim()
{
    { std::lock_guard<std::mutex> g(m_); closing_ = true; }
    quiesce();
    { std::lock_guard<std::mutex> g(g_pools_m); g_pools.erase(std::remove(g_pools.begin(), g_pools.end(), this), g_pools.end()); registered_ = false; }
    std::lock_guard<std::mutex> g(m_);
    closing_ = false;
    for (Stream &u : up) if (u) { (void)hipStreamSynchronize(u); u = Stream(); }   // (the copies out of busy pieces are done)
    made_ -= (uint32_t)(free_.size() + busy_.size());
    free_.clear(); busy_.clear(); kept_.clear(); pins_.clear();
}

}  // namespace mk
