// The compile-ahead pipeline of the streaming feeds (stream.inc, eval_stream.inc): the pieces of a feed are produced on worker
// threads ahead of the main thread, which takes them in order and runs them on the GPU.
//
//   PiecePipe pipe(n_pieces, n_threads, produce[, pick, run]);
//   for (i = 0 .. n_pieces) { rc = pipe.wait(i); ...run piece i...; pipe.consumed(i, rc); }
//
// produce(i) runs on a worker (any order, at most 2 x n_threads pieces ahead of the last consumed one: a compiled piece holds
// ~70 bytes per op) and returns the piece's code; an exception in it becomes `on_throw` for that piece.  With n_threads <= 1 there
// are no workers: wait(i) produces piece i inline.
// The optional side job is a second kind of work for a worker, on a piece that is produced but not yet taken: pick(pipe), called
// with the pipe's lock held, claims a piece (or returns NONE); run(i) does the work outside the lock; wait(i) does not return
// while it runs.  A side job goes before producing the next piece.
// The workers are stopped and joined by stop() and by the destructor, so on every way out -- an exception from the caller's
// loop included.  Declare the pipe after the state its callbacks use.
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace rv {

class PiecePipe {
  public:
    static constexpr size_t NONE = ~(size_t)0;
    using Produce = std::function<int(size_t)>;
    using Pick = std::function<size_t(const PiecePipe&)>;
    using Run = std::function<void(size_t)>;

    PiecePipe(size_t n_pieces, unsigned n_threads, int on_throw, Produce produce, Pick pick = nullptr, Run run = nullptr)
        : n_(n_pieces), window_(2 * (size_t)n_threads), on_throw_(on_throw), produce_(std::move(produce)), pick_(std::move(pick)), run_(std::move(run)), st_(n_pieces) {
        if (n_threads <= 1) return;
        try {
            for (unsigned t = 0; t < n_threads; t++) pool_.emplace_back([this] { work(); });
        } catch (...) {
            stop();
            throw;
        }
    }
    ~PiecePipe() { stop(); }
    PiecePipe(const PiecePipe&) = delete;
    PiecePipe& operator=(const PiecePipe&) = delete;

    // piece i is produced and no side job runs on it: it is the main thread's from here on
    int wait(size_t i) {
        if (pool_.empty() && !st_[i].ready) finish_piece(i, produce_guarded(i));
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return st_[i].ready && !st_[i].busy; });
        st_[i].taken = true;
        return st_[i].rc;
    }
    // the main thread is done with piece i; a failure stops the workers
    void consumed(size_t i, int rc) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            consumed_ = i + 1;
            if (rc) stop_ = true;
        }
        cv_.notify_all();
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread& t : pool_)
            if (t.joinable()) t.join();
    }
    // for pick (the lock is held)
    bool ready(size_t i) const { return st_[i].ready; }
    bool taken(size_t i) const { return st_[i].taken; }
    int rc(size_t i) const { return st_[i].rc; }
    size_t n_consumed() const { return consumed_; }

  private:
    struct State {
        int rc = 0;
        bool ready = false;  // produced
        bool taken = false;  // the main thread has it (or is past it)
        bool busy = false;   // a side job runs on it right now
    };
    int produce_guarded(size_t i) {
        try {
            return produce_(i);
        } catch (...) {
            return on_throw_;
        }
    }
    void finish_piece(size_t i, int rc) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            st_[i].rc = rc;
            st_[i].ready = true;
        }
        cv_.notify_all();
    }
    void work() {
        for (;;) {
            size_t i = NONE, side = NONE;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || (pick_ && (side = pick_(*this)) != NONE) || (next_ < n_ && next_ < consumed_ + window_); });
                if (stop_) return;
                if (side != NONE)
                    st_[side].busy = true;
                else
                    i = next_++;
            }
            if (side != NONE) {
                run_(side);
                {
                    std::lock_guard<std::mutex> lk(mu_);
                    st_[side].busy = false;
                }
                cv_.notify_all();
            } else {
                finish_piece(i, produce_guarded(i));
            }
        }
    }

    const size_t n_, window_;
    const int on_throw_;
    Produce produce_;
    Pick pick_;
    Run run_;
    std::vector<State> st_;
    std::mutex mu_;
    std::condition_variable cv_;
    size_t next_ = 0, consumed_ = 0;
    bool stop_ = false;
    std::vector<std::thread> pool_;
};

}  // namespace rv
