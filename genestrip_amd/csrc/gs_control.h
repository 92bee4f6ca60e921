// gs_control.h -- what a file-level call of the host layer (include/gshost.h) shares with the threads that watch or stop it: a
// cancel flag, the latest progress record and an optional callback.  Header-only, standard library only, no HIP and no other
// project header: gs_host.cpp includes it, and so does the stand-alone program tests/native/control_sanitize.cpp.
//
//   cancel flag   any thread sets it (cancel()), the loop's thread reads it after every chunk (cancelled())
//   record        published by the loop's thread (publish()), read from any thread (snapshot()) under one mutex: a reader sees a
//                 whole record, never half of one and half of another.  A lock per chunk -- a chunk is megabytes of text -- is
//                 nothing; a sequence lock would need fences that the thread sanitizer does not model.
//   callback      runs inside publish(), i.e. on the thread that made the file-level call, never on a worker and never twice at a
//                 time; a non-zero return sets the cancel flag.  every_ms > 0 drops calls that come sooner than that behind the
//                 last one, unless the record is forced (first / last record of a file, the closing record, the record of a stop).
#pragma once
#include <atomic>
#include <chrono>
#include <cstdint>
#include <mutex>

namespace gs_control {

// the layout of gs_host_progress (include/gshost.h; gs_host.cpp asserts that the two agree)
struct Record {
    int32_t file = 0, n_files = 0;
    int32_t file_done = 0;
    int32_t files_done = 0;
    int64_t file_bytes_done = 0, file_bytes_total = 0;
    int64_t file_reads = 0;
    int64_t total_bytes_done = 0, total_bytes_total = 0, total_reads = 0;
    double seconds_file = 0, seconds_total = 0;
};

typedef int (*Callback)(void *user, const Record *r);

class Control {
public:
    Control(Callback fn, void *user, int32_t every_ms) : fn_(fn), user_(user), every_ms_(every_ms) {}
    Control(const Control &) = delete;
    Control &operator=(const Control &) = delete;

    void cancel() { cancel_.store(true, std::memory_order_release); }
    bool cancelled() const { return cancel_.load(std::memory_order_acquire); }

    // the latest record (all zero before the first one) and the flag
    void snapshot(Record *out, bool *cancelled_out) const {
        {
            std::lock_guard<std::mutex> l(m_);
            *out = rec_;
        }
        if (cancelled_out) *cancelled_out = cancelled();
    }

    // The loop's thread only.  The record becomes the snapshot whether or not the callback runs.  ask = false: the record of a stop
    // -- the callback sees it, its answer no longer matters.  Returns cancelled().
    bool publish(const Record &r, bool force, bool ask = true) {
        {
            std::lock_guard<std::mutex> l(m_);
            rec_ = r;
        }
        if (fn_) {
            const int64_t now = now_ms();
            if (force || every_ms_ <= 0 || !called_ || now - last_call_ms_ >= every_ms_) {
                called_ = true;
                last_call_ms_ = now;
                const int rc = fn_(user_, &r);
                if (rc != 0 && ask) cancel();
            }
        }
        return cancelled();
    }

private:
    static int64_t now_ms() {
        return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    std::atomic<bool> cancel_{false};
    mutable std::mutex m_;
    Record rec_;
    const Callback fn_;
    void *const user_;
    const int32_t every_ms_;
    bool called_ = false;          // (loop's thread only, as last_call_ms_)
    int64_t last_call_ms_ = 0;
};

}  // namespace gs_control
