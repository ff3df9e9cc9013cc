// What a context keeps for the gzip inflater (gunzip.hip) between batches, in one owner that releases itself: device blocks,
// small page-locked staging, the page-locked pieces readers fill and the streams their copies run on.  The lock is the pool's
// own.  (Part of mk_internal.hpp, which includes it behind the owning types it is made of.)
#pragma once
#include <atomic>
#include <chrono>

namespace mk {

void pinned_free(void *p);
constexpr uint64_t kStagePiece = 16ull << 20;                         // (room for a run of eight 5 Mb genomes gzip'd: a copy per run)
constexpr uint32_t kStagePieces = 24;                                 // at most 384 MB of page-locked pieces per context

// what MIEKKI_VERBOSE shows of the pools, all contexts' together: device allocations made and their time, time readers stood
// waiting for a piece, time spent in mk_gz_put.  Timed: from its making to its scope's end into `us`, and one more into `n`
struct GzCounts {
    std::atomic<uint64_t> malloc_n{0}, malloc_us{0}, stage_waits{0}, stage_wait_us{0}, put_us{0};
    struct Timed {
        std::atomic<uint64_t> &us, *n;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~Timed() { if (n) ++*n; us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count(); }
    };
};
extern GzCounts g_gz_counts;

class GzPool : NoCopy {
public:
    // (a block is taken only for the role it was made for -- a batch's input + tokens, or its text: with one list for all, a text
    // block would take the place of a token block and the next batch allocate a new one, in the middle of the run: an
    // allocation of gigabytes while the device is busy took up to a second and a half)
    enum class Role { InputTokens, Text };
    int device = 0;                                                   // the context's (mk_create)
    // ---- device blocks, kept between batches (allocating and freeing tens of gigabytes per batch cost a second each)
    DevArray<uint8_t> take(Role role, uint64_t need);                 // the smallest kept block that fits, or a new one; empty: no memory
    void give(Role role, DevArray<uint8_t> &&blk);
    void make_ahead(uint64_t need_input, uint64_t need_text);         // on a thread of its own: blocks of these sizes, unless kept ones do
    void quiesce();                                                   // returns when no such thread is at work
    // ---- page-locked staging of a run's small copies: at least 1 MiB, powers of two; empty: none to be had
    PinnedArray<uint8_t> pin_take(uint64_t need);
    void pin_give(PinnedArray<uint8_t> &&pin);
    // ---- the pieces of kStagePiece bytes callers read their files into (mk_gz_stage), each with the event behind its copy
    // (pinned_alloc's memory -- huge pages, registered --, which a PinnedArray does not hold)
    struct PinnedFree { void operator()(void *p) const { pinned_free(p); } };
    struct Piece { std::unique_ptr<void, PinnedFree> mem; Event ev; };
    void *lend();                                                     // a piece into the caller's hands; null: all are there already
    bool claim(const void *data, Piece &piece, hipStream_t &up_k, uint32_t &k_up);   // the piece lent as `data`, and the upload stream its copy takes (up[k_up]); false: no piece
    void take_back(Piece &&piece, bool queued);                       // queued: its copy waits on the upload stream, ev behind it
    Stream up[4];                                                     // the upload streams, each made when first chosen (they take turns)
    bool use_device() const;                                          // the calling thread on the pool's device
    void trim();                                                      // everything kept goes back; pieces in callers' hands stay theirs
    ~GzPool() { trim(); }                                             // (pieces still out go too: nobody can return them afterwards.  The device is bound: mk_destroy)

private:
    friend uint64_t gz_release_idle_blocks();
    struct Block { DevArray<uint8_t> blk; Role role; };
    Block *fit(Role role, uint64_t need);
    DevArray<uint8_t> make(uint64_t need);
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<Block> kept_;
    uint32_t making_ = 0;                                             // block makers at work
    bool closing_ = false;                                            // no new one starts
    bool registered_ = false;                                         // among the pools that keep blocks (under the registry's lock, not m_)
    std::vector<PinnedArray<uint8_t>> pins_;
    std::vector<Piece> free_, held_;                                  // pieces at rest; in callers' hands
    std::deque<Piece> busy_;                                          // pieces whose copy is queued, oldest first
    uint32_t made_ = 0, up_next_ = 0;
};

}  // namespace mk
