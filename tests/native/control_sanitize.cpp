// control_sanitize.cpp -- genestrip_amd/csrc/gs_control.h under ThreadSanitizer / AddressSanitizer (tests/test_progress_cpu.py):
// one thread publishes records whose fields all follow from one counter, two threads take snapshots and check that every one of
// them is a whole record, one thread cancels; the publisher's callback sees every record in order, on the publisher's thread only.
// Prints "fails N"; exit status 0 when N is 0.
#include "../../genestrip_amd/csrc/gs_control.h"

#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

using gs_control::Control;
using gs_control::Record;

static Record record_of(int64_t i) {
    Record r;
    r.file = (int32_t)(i % 7);
    r.n_files = 7;
    r.file_done = (int32_t)(i & 1);
    r.files_done = (int32_t)(i % 5);
    r.file_bytes_done = i;
    r.file_bytes_total = 2 * i;
    r.file_reads = 3 * i;
    r.total_bytes_done = 5 * i;
    r.total_bytes_total = 7 * i;
    r.total_reads = 11 * i;
    r.seconds_file = (double)i * 0.5;
    r.seconds_total = (double)i * 0.25;
    return r;
}

static bool whole(const Record &r) {
    const int64_t i = r.file_bytes_done;
    const Record w = record_of(i);
    if (i == 0) return r.n_files == 0 || r.n_files == 7;  // (before the first record: all zero)
    return r.file == w.file && r.n_files == w.n_files && r.file_done == w.file_done && r.files_done == w.files_done &&
           r.file_bytes_total == w.file_bytes_total && r.file_reads == w.file_reads && r.total_bytes_done == w.total_bytes_done &&
           r.total_bytes_total == w.total_bytes_total && r.total_reads == w.total_reads && r.seconds_file == w.seconds_file &&
           r.seconds_total == w.seconds_total;
}

struct Seen {
    std::thread::id owner;
    int64_t calls = 0, last = 0, fails = 0;
};

static int on_record(void *user, const Record *r) {
    Seen *s = static_cast<Seen *>(user);
    if (std::this_thread::get_id() != s->owner) s->fails++;
    if (!whole(*r) || r->file_bytes_done <= s->last) s->fails++;
    s->last = r->file_bytes_done;
    s->calls++;
    return 0;
}

static int stop_at_10(void *, const Record *r) { return r->file_bytes_done == 10; }

int main() {
    int64_t fails = 0;
    const int64_t n = 300000;
    {
        Seen seen;
        Control c(on_record, &seen, 0);
        std::atomic<bool> done{false};
        std::atomic<int64_t> reader_fails{0}, snapshots{0}, stopped_at{0};
        std::thread pub([&] {
            seen.owner = std::this_thread::get_id();
            int64_t i = 1;
            for (; i <= n; i++)
                if (c.publish(record_of(i), false)) break;  // (the loop's thread looks at the flag after every record)
            stopped_at = i;
            done = true;
        });
        std::vector<std::thread> readers;
        for (int t = 0; t < 2; t++)
            readers.emplace_back([&] {
                int64_t last = 0;
                while (!done.load()) {
                    Record r;
                    bool stop = false;
                    c.snapshot(&r, &stop);
                    if (!whole(r) || r.file_bytes_done < last) reader_fails++;
                    last = r.file_bytes_done;
                    snapshots++;
                }
            });
        std::thread canceller([&] {
            for (;;) {  // half way through, or when the publisher is done before that
                Record r;
                c.snapshot(&r, nullptr);
                if (r.file_bytes_done >= n / 2 || done.load()) break;
                std::this_thread::yield();
            }
            c.cancel();
        });
        pub.join();
        canceller.join();
        for (auto &t : readers) t.join();
        Record r;
        bool stop = false;
        c.snapshot(&r, &stop);
        fails += reader_fails.load() + seen.fails;
        if (!stop || !c.cancelled()) fails++;
        if (stopped_at.load() < n / 2 || seen.calls != std::min(stopped_at.load(), n) || r.file_bytes_done != seen.last) fails++;
        printf("records %lld, callbacks %lld, snapshots %lld\n", (long long)stopped_at.load(), (long long)seen.calls, (long long)snapshots.load());
    }
    {  // a callback's non-zero answer sets the flag; the record of a stop is shown but not asked
        Control c(stop_at_10, nullptr, 0);
        int64_t i = 1;
        for (; i <= 100; i++)
            if (c.publish(record_of(i), false)) break;
        if (i != 10 || !c.cancelled()) fails++;
        Control d(stop_at_10, nullptr, 0);
        if (d.publish(record_of(10), true, false) || d.cancelled()) fails++;
    }
    {  // every_ms: a record that comes too soon reaches the snapshot but not the callback, unless it is forced
        Seen seen;
        seen.owner = std::this_thread::get_id();
        Control c(on_record, &seen, 60000);
        c.publish(record_of(1), false);
        c.publish(record_of(2), false);
        c.publish(record_of(3), true);
        Record r;
        c.snapshot(&r, nullptr);
        if (seen.calls != 2 || seen.last != 3 || r.file_bytes_done != 3 || seen.fails) fails++;
        c.publish(record_of(4), false);
        c.snapshot(&r, nullptr);
        if (seen.calls != 2 || r.file_bytes_done != 4) fails++;
    }
    {  // no callback: snapshots and the flag only
        Control c(nullptr, nullptr, 0);
        if (c.publish(record_of(5), true)) fails++;
        c.cancel();
        if (!c.publish(record_of(6), false)) fails++;
    }
    printf("fails %lld\n", (long long)fails);
    return fails ? 1 : 0;
}
