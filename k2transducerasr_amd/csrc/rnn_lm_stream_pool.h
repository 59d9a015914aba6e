// Neural LM shallow fusion in the STREAMING modified beam search: the device blocks the streams' hypotheses keep their LM state in between
// chunks, and their bookkeeping (include/k2hip.h "Neural LM shallow fusion in the streaming modified beam search"; the movers:
// rnn_lm_fuse.hip k_nlm_load_streams / k_nlm_store_streams).  Pure host code: tests/native/san_rnn_lm_stream_fusion_driver.cpp runs it
// under the sanitizers over a heap allocator.
//
// ONE BLOCK per fused stream, two halves of half_floats() floats each.  A half holds, for the K slots of the stream's beam,
//   state [K][L][2][H]   (h, c) of every LM layer: slot k, layer l, h at ((k L + l) 2) H, c one H further
//   rows  [K][V]         the LM's next-token log-probs of each slot, behind the states
// rounded up to a multiple of 4 floats, so both halves and every state row start on 16 bytes; the rows of slots k > 0 do not when V is
// not a multiple of 4.  A call READS the current half (none of a stream that has no state yet: the start state stands in) and WRITES the
// other one; the host flips the halves only after the call succeeded, so a failed call leaves the state the stream had.
//
// THE POOL belongs to the model and is shared (shared_ptr) with every stream that holds a block: the model's end (shutdown) frees all
// device memory and marks the pool gone, after which a stream's release or reset only forgets its handle -- it never names freed memory.
// Released blocks are kept for the next stream of the same size; blocks of another size (the LM was replaced) are freed on the next
// take.  Device allocation and release go through the two callbacks the owner gives: they run under the owner's engine lock
// (take, shutdown), never from release, which may come from any thread at any time.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define K2HIP_POOL_HD __host__ __device__
#else
#define K2HIP_POOL_HD
#endif

namespace k2hip {

struct NlmStreamLayout {
    int K, L, H, V;
    K2HIP_POOL_HD long long state_floats() const { return (long long)K * L * 2 * H; }
    K2HIP_POOL_HD long long state_off(int k, int l, int hc) const { return (((long long)k * L + l) * 2 + hc) * H; }
    K2HIP_POOL_HD long long row_off(int k) const { return state_floats() + (long long)k * V; }
    K2HIP_POOL_HD long long half_floats() const { return (state_floats() + (long long)K * V + 3) / 4 * 4; }
    K2HIP_POOL_HD long long block_floats() const { return 2 * half_floats(); }
};

class NlmStreamPool {
  public:
    using Alloc = std::function<void*(size_t)>;   // throws on failure
    using Free = std::function<void(void*)>;
    struct Stats {
        int64_t live = 0, bytes = 0;   // blocks streams hold; bytes of device memory the pool owns (held and spare blocks)
    };
    // A stream's handle: which block, which half is current, whether that half holds a state, and the LM it belongs to
    class Handle {
      public:
        Handle() = default;
        Handle(const Handle&) = delete;
        Handle& operator=(const Handle&) = delete;
        ~Handle() { release(); }
        bool held() const { return pool_ != nullptr; }
        bool has_state() const { return held() && has_; }
        uint64_t lm_serial() const { return serial_; }
        // the LM-serial check: a held block carries state of ONE setting of the LM; a call under another setting must not read it
        bool carries(uint64_t serial) const { return held() && serial_ == serial; }
        // the half this call reads (null: no state yet, or the model is gone) and the half it writes
        const float* read_half() const { return has_state() && !pool_->gone() ? base_ + (size_t)cur_ * half_ : nullptr; }
        float* write_half() const { return held() && !pool_->gone() ? base_ + (size_t)(cur_ ^ 1) * half_ : nullptr; }
        // after a call that succeeded: what it wrote is the state
        void flip() {
            if (!held()) return;
            cur_ ^= 1;
            has_ = true;
        }
        // back to the start state; the block returns to the pool (or is forgotten when the model is gone)
        void release() {
            if (!pool_) return;
            pool_->give_back(base_, floats_);
            pool_.reset();
            base_ = nullptr;
            has_ = false;
            cur_ = 0;
            serial_ = 0;
        }

      private:
        friend class NlmStreamPool;
        std::shared_ptr<NlmStreamPool> pool_;
        float* base_ = nullptr;
        size_t half_ = 0, floats_ = 0;
        int cur_ = 0;
        bool has_ = false;
        uint64_t serial_ = 0;
    };

    NlmStreamPool(Alloc a, Free f) : alloc_(std::move(a)), free_(std::move(f)) {}
    ~NlmStreamPool() { shutdown(); }
    NlmStreamPool(const NlmStreamPool&) = delete;
    NlmStreamPool& operator=(const NlmStreamPool&) = delete;

    // a block of layout `lay` for handle `h` (which holds none), noted as belonging to LM `serial`; self: the owner's shared_ptr to
    // this pool.  The owner's lock is held.  Throws what the allocator throws; the handle then holds nothing.
    static void take(const std::shared_ptr<NlmStreamPool>& self, Handle& h, const NlmStreamLayout& lay, uint64_t serial) {
        NlmStreamPool& p = *self;
        const size_t floats = (size_t)lay.block_floats();
        float* base = nullptr;
        std::vector<std::pair<float*, size_t>> stale;
        {
            std::lock_guard<std::mutex> lk(p.mu_);
            for (size_t i = 0; i < p.spare_.size();) {
                if (p.spare_[i].second == floats && !base) {
                    base = p.spare_[i].first;
                    p.spare_.erase(p.spare_.begin() + (long)i);
                } else if (p.spare_[i].second != floats) {   // (of an LM that was replaced)
                    stale.push_back(p.spare_[i]);
                    p.spare_.erase(p.spare_.begin() + (long)i);
                } else {
                    i++;
                }
            }
        }
        for (auto& s : stale) {
            p.free_(s.first);
            std::lock_guard<std::mutex> lk(p.mu_);
            p.bytes_ -= (int64_t)(s.second * sizeof(float));
        }
        if (!base) {
            base = static_cast<float*>(p.alloc_(floats * sizeof(float)));
            std::lock_guard<std::mutex> lk(p.mu_);
            p.bytes_ += (int64_t)(floats * sizeof(float));
        }
        {
            std::lock_guard<std::mutex> lk(p.mu_);
            p.live_++;
            p.held_.emplace_back(base, floats);
        }
        h.pool_ = self;
        h.base_ = base;
        h.half_ = (size_t)lay.half_floats();
        h.floats_ = floats;
        h.cur_ = 0;
        h.has_ = false;
        h.serial_ = serial;
    }
    // the model's end: every block, held or spare, is freed; handles that still exist only forget theirs from now on.  The owner's lock
    // is held and the device is idle.
    void shutdown() {
        std::vector<std::pair<float*, size_t>> all;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (gone_) return;
            gone_ = true;
            all.swap(spare_);
            all.insert(all.end(), held_.begin(), held_.end());
            held_.clear();
            bytes_ = 0;
        }
        for (auto& b : all) {
            try {
                free_(b.first);
            } catch (...) {
            }
        }
    }
    bool gone() const {
        std::lock_guard<std::mutex> lk(mu_);
        return gone_;
    }
    Stats stats() const {
        std::lock_guard<std::mutex> lk(mu_);
        return Stats{live_, bytes_};
    }

  private:
    void give_back(float* base, size_t floats) {
        std::lock_guard<std::mutex> lk(mu_);
        live_--;
        if (gone_) return;   // (freed with the model)
        for (size_t i = 0; i < held_.size(); i++)
            if (held_[i].first == base) {
                held_.erase(held_.begin() + (long)i);
                break;
            }
        spare_.emplace_back(base, floats);
    }
    friend class Handle;

    Alloc alloc_;
    Free free_;
    mutable std::mutex mu_;
    std::vector<std::pair<float*, size_t>> spare_, held_;
    int64_t live_ = 0, bytes_ = 0;
    bool gone_ = false;
};

}  // namespace k2hip
